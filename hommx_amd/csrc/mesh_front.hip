// mesh_front.hip -- cell problems on an unstructured periodic micro mesh: batched frontal elimination.
//
// All cells of a batch share the mesh, the elimination order and therefore the whole symbolic phase; only the coefficients (and M)
// differ.  The host validates the mesh, orders the periodic nodes (unless the caller gives an order: the narrower of reverse Cuthill-McKee and a coordinate sweep), gives
// every node a front slot for its lifetime (lowest free slot first, so the slots used never exceed the front width), and groups
// the elements by the step that assembles them, coloured so that no two elements of a group share a node.
//
// The kernel eliminates  [[K, B], [B^T, 0]]  node by node, one workgroup per macro cell.  The front is the packed lower triangle of
// the symmetric (t + W) x (t + W) matrix in LDS: rows 0..t-1 are the border (the t canonical loads), row t + slot * bs + c the
// unknown c of the node in `slot`.  Step k assembles the element matrices of the elements whose first node in the order is node k
// (formed on the device from the cell's coefficient and M: K_rs = vol s_r^T C s_s, B_rm = -vol (C s_r)_m with s_r the strain of
// local dof r in the basis of the canonical loads), then eliminates the bs unknowns of node k (rank-1 updates of the active part of
// the front; the pivot's row and column are cleared so its slot can be reused).  What is left in the border is -B^T K^-1 B;
// A_H = C0 + that, C0 = sum vol C.  The last node of the order is pinned: its unknowns never enter the front.
//
// Correctors: every pivot's column (before the update) goes to a per-chunk HBM arena; a second kernel substitutes backwards through
// it and removes the mean per component.
//
// Load solves: the arena is a complete L D L^T record of K, so a right-hand side that is not one of the canonical loads needs no
// second elimination.  k_mesh_front_rhs assembles the loads of a LoadOverride per node, carries them forwards through the stored
// columns and substitutes backwards as k_mesh_backsub does (mesh_load_correctors; the arena must still hold the cells' columns).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>
#include <string>
#include <vector>

#include "host_common.h"
#include "kernels.h"
#include "mesh_elem.h"
#include "mesh_front.h"

namespace hommx {

namespace {
constexpr int kThreads = 256;
constexpr int kRed = 21;  // t (t + 1) / 2 for t <= 6: the C0 partial sums
// k_mesh_front_rhs: a work item is one load on one segment of kSeg front rows, taken by half a wavefront
constexpr int kSeg = 32, kHalves = kThreads / kSeg, kMaxSeg = HOMMX_MESH_MAX_FRONT / kSeg;
}  // namespace

// device view of the symbolic phase (all arrays on the plan's device)
struct MeshDev {
  int n_el, n_nodes, n_steps, S;  // S = t + front width: rows of the largest front
  const double* grads;            // [n_el][dim+1][dim]  P1 gradients in the caller's element order (the plan's MeshGeomDev block)
  const double* vol;              // [n_el]
  const int* el_slot;             // [n_el][dim+1]  front slot of every vertex's node, -1 for the pinned node
  const int* el_seq;              // elements in assembly order
  const int* grp_ptr;             // [n_grp + 1] groups of el_seq (pairwise node-disjoint elements)
  const int* step_grp;            // [n_steps + 1] groups of each step
  const int* step_slot;           // [n_steps] slot of the node eliminated at the step
  const int* step_S;              // [n_steps] rows of the front that are in use at the step
  const long long* piv_off;       // [n_steps * bs + 1] offset of every pivot's column in a cell's arena
  const int* step_node;           // [n_steps] node eliminated at the step
  const int* owner;               // [n_steps][W / bs] node in every slot at the step (-1: free)
};

// node -> (element, vertex) incidence on the device: what k_mesh_front_rhs assembles a node's load entries through.  Kept out of
// MeshDev, whose layout is part of the kernel arguments of k_mesh_front and k_mesh_backsub
struct MeshInc {
  const int* ptr;  // [n_nodes + 1]
  const int* ent;  // [n_el (dim + 1)] element * 4 + vertex; the entries of a node ascend by element
  int pinned;      // the node whose unknowns never enter the front
};

struct MeshPlan {
  int dim = 0, kind = 0, bs = 1, t = 0, n_comp = 0;
  int64_t n_nodes = 0, n_el = 0;
  int32_t front_width = 0;
  double flops = 0.0;
  int n_steps = 0, nslots = 0, S = 0;
  std::vector<int> order, pos;
  std::vector<int> el_slot, el_seq, grp_ptr, step_grp, step_slot, step_S, step_node, owner;
  std::vector<long long> piv_off;
  std::vector<int> inc_ptr, inc_ent;
  MeshDev dev{};
  MeshInc inc{};
  void* d_tables = nullptr;  // one allocation holds every device table of the symbolic phase
  double* d_arena = nullptr;
  int32_t* d_binfo = nullptr;
  long long cap_arena_cells = 0;
  // cells whose columns the arena holds, counted from the first cell of the last corrector call: all of them when that call ran as one
  // arena chunk, none when it walked several (the arena then holds the last chunk's alone)
  long long arena_valid = 0;
  std::string detail;
};

// ------------------------------------------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }  // packed lower triangle, i >= j

template <int DIM, int KIND>
__global__ void __launch_bounds__(kThreads) k_mesh_front(MeshDev G, const double* __restrict__ coef, const double* __restrict__ Mall,
                                                         double* __restrict__ out, int32_t* __restrict__ info, double* __restrict__ arena,
                                                         long long arena_per_cell) {
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, BS = ks.bs, NCOMP = ks.n_comp;
  constexpr int NV = DIM + 1, NL = NV * BS;
  constexpr int NKK = NL * (NL + 1) / 2, NE = NKK + NL * T;  // front entries one element adds (K lower triangle, B)
  extern __shared__ double smem[];
  const int S = G.S;
  double* F = smem;                  // packed front, S (S + 1) / 2
  double* cp = F + S * (S + 1) / 2;  // pivot column, S
  double* red = cp + S;              // [kThreads / 64][kRed]
  const int tid = threadIdx.x;
  const long long cell = blockIdx.x;
  const double* cc = coef + cell * (long long)G.n_el * NCOMP;
  const double* M = Mall ? Mall + cell * DIM * DIM : nullptr;
  double* ar = arena ? arena + (long long)blockIdx.x * arena_per_cell : nullptr;

  for (int q = tid; q < S * (S + 1) / 2; q += kThreads) F[q] = 0.0;
  int32_t bad = 0;
  __syncthreads();
  int piv = 0;
  for (int k = 0; k < G.n_steps && !bad; ++k) {
    // assemble the elements whose first node is node k, one node-disjoint group at a time
    for (int g = G.step_grp[k]; g < G.step_grp[k + 1]; ++g) {
      const int e0 = G.grp_ptr[g], ne = G.grp_ptr[g + 1] - e0;
      for (int q = tid; q < ne * NE; q += kThreads) {
        const int el = G.el_seq[e0 + q / NE];
        int r = q % NE, s2 = -1, m = -1;
        if (r < NKK) {
          int rr = 0;
          while (r > rr) {
            r -= rr + 1;
            ++rr;
          }
          s2 = r;
          r = rr;
        } else {
          m = (r - NKK) % T;
          r = (r - NKK) / T;
        }
        const int sr = G.el_slot[el * NV + r / BS];
        if (sr < 0) continue;
        const int fi = T + sr * BS + r % BS;
        int fj = m;
        if (s2 >= 0) {
          const int ss = G.el_slot[el * NV + s2 / BS];
          if (ss < 0) continue;
          fj = T + ss * BS + s2 % BS;
        }
        double C[T][T];
        material<DIM, KIND>(cc + (long long)el * NCOMP, C);
        double a[T], Ca[T];
        strain<DIM, KIND>(G.grads + ((long long)el * NV + r / BS) * DIM, M, r % BS, a);
#pragma unroll
        for (int i = 0; i < T; ++i) {
          double v = 0.0;
#pragma unroll
          for (int j = 0; j < T; ++j) v += C[i][j] * a[j];
          Ca[i] = v;
        }
        const double vol = G.vol[el];
        double val;
        if (s2 >= 0) {
          double b[T];
          strain<DIM, KIND>(G.grads + ((long long)el * NV + s2 / BS) * DIM, M, s2 % BS, b);
          double v = 0.0;
#pragma unroll
          for (int i = 0; i < T; ++i) v += Ca[i] * b[i];
          val = vol * v;
        } else {
          double v = 0.0;
#pragma unroll
          for (int i = 0; i < T; ++i) v = i == m ? Ca[i] : v;
          val = -vol * v;
        }
        F[fi >= fj ? tri(fi, fj) : tri(fj, fi)] += val;
      }
      __syncthreads();
    }
    // eliminate the bs unknowns of node k
    const int Sk = G.step_S[k];
    for (int c = 0; c < BS; ++c, ++piv) {
      const int p = T + G.step_slot[k] * BS + c;
      for (int i = tid; i < Sk; i += kThreads) cp[i] = F[i >= p ? tri(i, p) : tri(p, i)];
      __syncthreads();
      const double d = cp[p];
      if (!(d > 0.0) || !isfinite(d)) {  // uniform across the workgroup: every thread read the same cp[p]
        bad = piv + 1;
        break;
      }
      if (ar)
        for (int i = tid; i < Sk; i += kThreads) ar[G.piv_off[piv] + i] = cp[i];
      const double rd = 1.0 / d;
      const int nq = Sk * (Sk + 1) / 2;
      // walk the packed triangle: entry q = tri(i, j); (i, j) advanced incrementally by kThreads entries
      int i = (int)((sqrt(8.0 * tid + 1.0) - 1.0) * 0.5);
      while (tri(i + 1, 0) <= tid) ++i;
      while (tri(i, 0) > tid) --i;
      int j = tid - tri(i, 0);
      for (int q = tid; q < nq; q += kThreads) {
        if (i == p || j == p)
          F[q] = 0.0;
        else
          F[q] -= cp[i] * (cp[j] * rd);
        j += kThreads;
        while (j > i) {
          j -= i + 1;
          ++i;
        }
      }
      __syncthreads();
    }
  }

  // C0 = sum over the elements of vol C (fixed order per thread, then a fixed reduction tree: deterministic)
  double c0[kRed];
#pragma unroll
  for (int q = 0; q < kRed; ++q) c0[q] = 0.0;
  for (int el = tid; el < G.n_el; el += kThreads) {
    double C[T][T];
    material<DIM, KIND>(cc + (long long)el * NCOMP, C);
    const double vol = G.vol[el];
    int q = 0;
#pragma unroll
    for (int m = 0; m < T; ++m)
#pragma unroll
      for (int n = 0; n <= m; ++n, ++q) c0[q] += vol * C[m][n];
  }
#pragma unroll
  for (int q = 0; q < T * (T + 1) / 2; ++q) {
    double v = c0[q];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
    if ((tid & 63) == 0) red[(tid >> 6) * kRed + q] = v;
  }
  __syncthreads();
  if (tid < T * T) {
    const int m = tid / T, n = tid % T;
    const int q = m >= n ? tri(m, n) : tri(n, m);
    double v = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) v += red[w * kRed + q];
    out[cell * T * T + tid] = v + F[q];
  }
  if (tid == 0 && info) info[cell] = bad;
}

// back substitution through the arena, then the mean removed per component; corr[cell][t][n_nodes * bs]
template <int T, int BS>
__global__ void __launch_bounds__(kThreads) k_mesh_backsub(MeshDev G, const double* __restrict__ arena, long long arena_per_cell,
                                                           const int32_t* __restrict__ info, double* __restrict__ corr) {
  __shared__ double part[kThreads / 64][T];
  const int tid = threadIdx.x;
  const long long cell = blockIdx.x;
  const double* ar = arena + cell * arena_per_cell;
  const long long nu = (long long)G.n_nodes * BS;
  double* x = corr + cell * T * nu;
  const int W = (G.S - T) / BS;  // slots
  const bool ok = info[cell] == 0;
  for (long long q = tid; q < T * nu; q += kThreads) x[q] = ok ? 0.0 : NAN;
  __threadfence_block();
  __syncthreads();
  if (ok) {
    for (int k = G.n_steps - 1; k >= 0; --k) {
      const int Sk = G.step_S[k];
      for (int c = BS - 1; c >= 0; --c) {
        const int piv = k * BS + c;
        const double* col = ar + G.piv_off[piv];
        const int p = T + G.step_slot[k] * BS + c;
        double acc[T];
#pragma unroll
        for (int m = 0; m < T; ++m) acc[m] = 0.0;
        for (int i = T + tid; i < Sk; i += kThreads) {
          if (i == p) continue;
          const int nd = G.owner[(long long)k * W + (i - T) / BS];
          const double v = col[i];
          if (nd < 0 || v == 0.0) continue;
          const long long u = (long long)nd * BS + (i - T) % BS;
#pragma unroll
          for (int m = 0; m < T; ++m) acc[m] += v * x[m * nu + u];
        }
#pragma unroll
        for (int m = 0; m < T; ++m) {
          double v = acc[m];
#pragma unroll
          for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
          if ((tid & 63) == 0) part[tid >> 6][m] = v;
        }
        __syncthreads();
        if (tid < T) {
          double s = 0.0;
          for (int w = 0; w < kThreads / 64; ++w) s += part[w][tid];
          x[tid * nu + (long long)G.step_node[k] * BS + c] = (col[tid] - s) / col[p];
        }
        __threadfence_block();
        __syncthreads();
      }
    }
    // mean-free per component
    for (int mc = 0; mc < T * BS; ++mc) {
      const int m = mc / BS, c = mc % BS;
      double s = 0.0;
      for (long long nd = tid; nd < G.n_nodes; nd += kThreads) s += x[m * nu + nd * BS + c];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) s += __shfl_down(s, o, 64);
      if ((tid & 63) == 0) part[tid >> 6][0] = s;
      __syncthreads();
      double tot = 0.0;
      for (int w = 0; w < kThreads / 64; ++w) tot += part[w][0];
      const double mean = tot / (double)G.n_nodes;
      for (long long nd = tid; nd < G.n_nodes; nd += kThreads) x[m * nu + nd * BS + c] -= mean;
      __syncthreads();
    }
  }
}

// Correctors of user loads by substitution on the arena k_mesh_front has just filled: K chi_l = -f^l for the loads l < n_loads of `lo`,
// in place on rows l < n_loads of corr[cell][t][n_nodes * bs] (the rows behind them are not written).  One workgroup per macro cell.
//   assemble   r[l][i bs + al] = -sum_{K ni i} |K| P^l_K . strain(g_{a(i,K)}, M, al), one thread per node over its incidence list in
//              order (the arithmetic of k_assemble_loads_mesh); the pinned node's entries are zero and stay so
//   forward    pivots in elimination order: y = r at the pivot, r[owner(i)] -= col[i] (y / d) for the other front rows i of the stored
//              column (distinct rows are distinct entries: no atomics; rows the elimination cleared hold 0 and are skipped)
//   backward   k_mesh_backsub's recurrence with y in place of the border entry: x_p = (y_p - sum_{i != p} col[i] x_owner(i)) / d
// and the mean removed per component.  The lanes are spread over (front row x load): an item is one load on one segment of kSeg front
// rows, the kHalves half-waves take the items in turn.  A load's sum over the rows of a pivot is formed per segment by a butterfly and
// over the segments in order, so a load's corrector does not depend on how many loads the call has.  The vectors stay in global memory
// (n_nodes is not bounded by the front width); within the workgroup they are ordered by fences and barriers, as in k_mesh_backsub.
template <int DIM, int KIND>
__global__ void __launch_bounds__(kThreads) k_mesh_front_rhs(MeshDev G, MeshInc I, const double* __restrict__ arena, long long arena_per_cell,
                                                             const int32_t* __restrict__ info, LoadOverride lo, const double* __restrict__ Mall,
                                                             double* corr) {
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, BS = ks.bs, NV = DIM + 1;
  __shared__ double part[kMaxSeg][T];
  __shared__ double wsum[kThreads / 64];
  const int tid = threadIdx.x, lane = tid % kSeg, half = tid / kSeg;
  const long long cell = blockIdx.x;
  const double* ar = arena + cell * arena_per_cell;
  const long long nu = (long long)G.n_nodes * BS;
  double* x = corr + cell * T * nu;
  const int nl = lo.n_loads;
  const int W = (G.S - T) / BS;  // slots
  if (info[cell] != 0) {         // uniform across the workgroup
    for (long long q = tid; q < nl * nu; q += kThreads) x[q] = NAN;
    return;
  }

  // assemble
  {
    const double* M = Mall ? Mall + cell * DIM * DIM : nullptr;
    const double* P = lo.P + (lo.per_cell ? cell * nl : 0) * (long long)G.n_el * T;
    for (int i = tid; i < G.n_nodes; i += kThreads) {
      double acc[T][BS];
#pragma unroll
      for (int m = 0; m < T; ++m)
#pragma unroll
        for (int b = 0; b < BS; ++b) acc[m][b] = 0.0;
      const int q1 = i == I.pinned ? 0 : I.ptr[i + 1];
      for (int q = I.ptr[i]; q < q1; ++q) {
        const unsigned ent = (unsigned)I.ent[q];
        const long long el = ent >> 2;
        const double vol = G.vol[el];
        const double* gr = G.grads + (el * NV + (ent & 3)) * DIM;
#pragma unroll
        for (int b = 0; b < BS; ++b) {
          double sb[T];
          strain<DIM, KIND>(gr, M, b, sb);
#pragma unroll
          for (int m = 0; m < T; ++m)
            if (m < nl) {
              const double* __restrict__ pk = P + ((long long)m * G.n_el + el) * T;
              double v = 0.0;
#pragma unroll
              for (int k = 0; k < T; ++k) v += pk[k] * sb[k];
              acc[m][b] -= vol * v;
            }
        }
      }
#pragma unroll
      for (int m = 0; m < T; ++m)
        if (m < nl) {
#pragma unroll
          for (int b = 0; b < BS; ++b) x[m * nu + (long long)i * BS + b] = acc[m][b];
        }
    }
  }
  __threadfence_block();
  __syncthreads();

  // forward
  for (int k = 0; k < G.n_steps; ++k) {
    const int Sk = G.step_S[k], nseg = (Sk - T + kSeg - 1) / kSeg, nitem = nseg * nl;
    const long long un = (long long)G.step_node[k] * BS;
    const int* own = G.owner + (long long)k * W;
    for (int c = 0; c < BS; ++c) {
      const double* col = ar + G.piv_off[k * BS + c];
      const int p = T + G.step_slot[k] * BS + c;
      const double d = col[p];
      for (int q = half; q < nitem; q += kHalves) {
        const int l = q / nseg, i = T + (q - l * nseg) * kSeg + lane;
        if (i >= Sk || i == p) continue;
        const int nd = own[(i - T) / BS];
        const double v = col[i];
        if (nd < 0 || v == 0.0) continue;
        double* xl = x + l * nu;
        xl[(long long)nd * BS + (i - T) % BS] -= v * (xl[un + c] / d);
      }
      __threadfence_block();
      __syncthreads();
    }
  }

  // backward
  for (int k = G.n_steps - 1; k >= 0; --k) {
    const int Sk = G.step_S[k], nseg = (Sk - T + kSeg - 1) / kSeg, nitem = nseg * nl;
    const long long un = (long long)G.step_node[k] * BS;
    const int* own = G.owner + (long long)k * W;
    for (int c = BS - 1; c >= 0; --c) {
      const double* col = ar + G.piv_off[k * BS + c];
      const int p = T + G.step_slot[k] * BS + c;
      for (int q0 = 0; q0 < nitem; q0 += kHalves) {  // the same trips for every half-wave: the butterfly runs in uniform control flow
        const int q = q0 + half;
        const bool active = q < nitem;
        const int l = active ? q / nseg : 0, seg = q - l * nseg, i = T + seg * kSeg + lane;
        double a = 0.0;
        if (active && i < Sk && i != p) {
          const int nd = own[(i - T) / BS];
          const double v = col[i];
          if (nd >= 0 && v != 0.0) a = v * x[l * nu + (long long)nd * BS + (i - T) % BS];
        }
#pragma unroll
        for (int o = kSeg / 2; o >= 1; o >>= 1) a += __shfl_xor(a, o, kSeg);
        if (active && lane == 0) part[seg][l] = a;
      }
      __syncthreads();
      if (tid < nl) {
        double s = 0.0;
        for (int seg = 0; seg < nseg; ++seg) s += part[seg][tid];
        x[tid * nu + un + c] = (x[tid * nu + un + c] - s) / col[p];
      }
      __threadfence_block();
      __syncthreads();
    }
  }

  // mean-free per component
  for (int lc = 0; lc < nl * BS; ++lc) {
    const int l = lc / BS, c = lc % BS;
    double s = 0.0;
    for (long long nd = tid; nd < G.n_nodes; nd += kThreads) s += x[l * nu + nd * BS + c];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_down(s, o, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = s;
    __syncthreads();
    double tot = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) tot += wsum[w];
    const double mean = tot / (double)G.n_nodes;
    for (long long nd = tid; nd < G.n_nodes; nd += kThreads) x[l * nu + nd * BS + c] -= mean;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// host side: validation and symbolic phase
// ------------------------------------------------------------------------------------------------------------------------------

namespace {

// reverse Cuthill-McKee on the node graph, from a pseudo-peripheral node (a few BFS sweeps from a node of least degree)
std::vector<int> rcm_order(int n, const std::vector<int>& ptr, const std::vector<int>& adj) {
  std::vector<int> deg(n), lvl(n), out;
  for (int v = 0; v < n; ++v) deg[v] = ptr[v + 1] - ptr[v];
  auto bfs = [&](int s, int& far) {
    std::fill(lvl.begin(), lvl.end(), -1);
    std::vector<int> q{s};
    lvl[s] = 0;
    for (size_t h = 0; h < q.size(); ++h)
      for (int e = ptr[q[h]]; e < ptr[q[h] + 1]; ++e)
        if (lvl[adj[e]] < 0) {
          lvl[adj[e]] = lvl[q[h]] + 1;
          q.push_back(adj[e]);
        }
    far = q.back();
    for (int v : q)
      if (lvl[v] == lvl[far] && deg[v] < deg[far]) far = v;
    return lvl[far];
  };
  int s = (int)(std::min_element(deg.begin(), deg.end()) - deg.begin());
  int far = s, ecc = bfs(s, far);
  for (int it = 0; it < 4; ++it) {
    int f2 = far;
    const int e2 = bfs(far, f2);
    if (e2 <= ecc) break;
    s = far;
    ecc = e2;
    far = f2;
  }
  std::vector<char> seen(n, 0);
  out.reserve(n);
  out.push_back(s);
  seen[s] = 1;
  std::vector<int> nb;
  for (size_t h = 0; h < out.size(); ++h) {
    nb.clear();
    for (int e = ptr[out[h]]; e < ptr[out[h] + 1]; ++e)
      if (!seen[adj[e]]) {
        seen[adj[e]] = 1;
        nb.push_back(adj[e]);
      }
    std::stable_sort(nb.begin(), nb.end(), [&](int a, int b) { return deg[a] < deg[b]; });
    out.insert(out.end(), nb.begin(), nb.end());
  }
  std::reverse(out.begin(), out.end());
  return out;
}

// front width, in nodes, of an elimination order (the symbolic simulation below, counts only): node v is in the front from the step
// that assembles its first element to its own step; the last node of the order never enters
int width_of(const std::vector<int>& order, const hommx_mesh_desc* d) {
  const int n = (int)d->n_nodes, ne = (int)d->n_el, nv = d->dim + 1;
  std::vector<int> pos(n), birth(n, n), delta(n + 1, 0);
  for (int k = 0; k < n; ++k) pos[order[k]] = k;
  for (int e = 0; e < ne; ++e) {
    int f = n;
    for (int a = 0; a < nv; ++a) f = std::min(f, pos[d->el_nodes[e * nv + a]]);
    for (int a = 0; a < nv; ++a) birth[d->el_nodes[e * nv + a]] = std::min(birth[d->el_nodes[e * nv + a]], f);
  }
  for (int v = 0; v < n; ++v)
    if (v != order[n - 1]) {
      ++delta[birth[v]];
      --delta[pos[v] + 1];
    }
  int w = 0, run = 0;
  for (int k = 0; k < n; ++k) w = std::max(w, run += delta[k]);
  return w;
}

// coordinate sweep: nodes sorted by their (folded) coordinate along `axis`, ties by the other axes -- two cross-sections wide on a
// periodic mesh, where the level sets of a breadth-first search from one node grow to twice that
std::vector<int> sweep_order(int n, int dim, const std::vector<double>& y, int axis) {
  std::vector<int> ord(n);
  for (int v = 0; v < n; ++v) ord[v] = v;
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) {
    for (int j = 0; j < dim; ++j) {
      const int c = (axis + j) % dim;
      const double ya = y[(size_t)a * dim + c], yb = y[(size_t)b * dim + c];
      if (std::fabs(ya - yb) > 1e-9) return ya < yb;
    }
    return false;
  });
  return ord;
}

}  // namespace

int mesh_check(const hommx_mesh_desc* d, MeshGeom* g) {
  if (!d) return fail(HOMMX_EINVAL, "null descriptor");
  if (d->dim != 2 && d->dim != 3) return fail(HOMMX_EINVAL, "dim must be 2 or 3, got %d", d->dim);
  if (d->kind < 0 || d->kind > 3) return fail(HOMMX_EINVAL, "unknown kind %d", d->kind);
  if (d->n_nodes < 2 || d->n_nodes > 0x3fffffffll) return fail(HOMMX_EINVAL, "n_nodes must be in [2, 2^30), got %lld", (long long)d->n_nodes);
  if (d->n_el < 1 || d->n_el > 0x3fffffffll) return fail(HOMMX_EINVAL, "n_el must be in [1, 2^30), got %lld", (long long)d->n_el);
  if (!d->el_nodes || !d->el_x) return fail(HOMMX_EINVAL, "null el_nodes / el_x");
  const int dim = d->dim, nv = dim + 1;
  const int n = (int)d->n_nodes, ne = (int)d->n_el;

  // topology
  std::vector<int> used(n, 0);
  for (int e = 0; e < ne; ++e)
    for (int a = 0; a < nv; ++a) {
      const int v = d->el_nodes[e * nv + a];
      if (v < 0 || v >= n) return fail(HOMMX_EINVAL, "element %d: node %d out of range [0, %d)", e, v, n);
      for (int b = 0; b < a; ++b)
        if (d->el_nodes[e * nv + b] == v)
          return fail(HOMMX_EINVAL, "element %d: periodic node %d appears twice (the mesh is too coarse for its periodic folding)", e, v);
      used[v] = 1;
    }
  for (int v = 0; v < n; ++v)
    if (!used[v]) return fail(HOMMX_EINVAL, "node %d belongs to no element", v);

  // geometry: P1 gradients and volumes from the unfolded coordinates
  g->grads.assign((size_t)ne * nv * dim, 0.0);
  g->vol.assign(ne, 0.0);
  double vsum = 0.0;
  for (int e = 0; e < ne; ++e) {
    const double* X = d->el_x + (size_t)e * nv * dim;
    double J[3][3] = {}, Ji[3][3] = {};
    for (int r = 0; r < dim; ++r)
      for (int c = 0; c < dim; ++c) J[r][c] = X[(r + 1) * dim + c] - X[c];
    double det;
    if (dim == 2) {
      det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
      Ji[0][0] = J[1][1] / det;
      Ji[0][1] = -J[0][1] / det;
      Ji[1][0] = -J[1][0] / det;
      Ji[1][1] = J[0][0] / det;
    } else {
      det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
            J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
          const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
          Ji[r][c] = (J[r1][c1] * J[r2][c2] - J[r1][c2] * J[r2][c1]) / det;  // adjugate / det
        }
    }
    const double v = std::fabs(det) / (dim == 2 ? 2.0 : 6.0);
    if (!(v > 1e-10 / ne) || !std::isfinite(v)) return fail(HOMMX_EINVAL, "element %d is degenerate (volume %.3g)", e, v);
    g->vol[e] = v;
    vsum += v;
    // grad phi_a = column a - 1 of J^-1 (a >= 1), grad phi_0 = -sum of the others
    double* gr = g->grads.data() + (size_t)e * nv * dim;
    for (int a = 1; a < nv; ++a)
      for (int c = 0; c < dim; ++c) {
        gr[a * dim + c] = Ji[c][a - 1];
        gr[c] -= Ji[c][a - 1];
      }
  }
  if (!(std::fabs(vsum - 1.0) <= 1e-10))
    return fail(HOMMX_EINVAL, "element volumes sum to %.15g, expected 1 (the unit cell)", vsum);

  // node graph (for the order and the connectivity check)
  std::vector<int>& ptr = g->ptr;
  std::vector<int>& adj = g->adj;
  ptr.assign(n + 1, 0);
  adj.clear();
  {
    std::vector<std::vector<int>> nb(n);
    for (int e = 0; e < ne; ++e)
      for (int a = 0; a < nv; ++a)
        for (int b = 0; b < nv; ++b)
          if (a != b) nb[d->el_nodes[e * nv + a]].push_back(d->el_nodes[e * nv + b]);
    for (int v = 0; v < n; ++v) {
      std::sort(nb[v].begin(), nb[v].end());
      nb[v].erase(std::unique(nb[v].begin(), nb[v].end()), nb[v].end());
      ptr[v + 1] = ptr[v] + (int)nb[v].size();
      adj.insert(adj.end(), nb[v].begin(), nb[v].end());
    }
  }
  {
    std::vector<char> seen(n, 0);
    std::vector<int> q{0};
    seen[0] = 1;
    for (size_t h = 0; h < q.size(); ++h)
      for (int e = ptr[q[h]]; e < ptr[q[h] + 1]; ++e)
        if (!seen[adj[e]]) {
          seen[adj[e]] = 1;
          q.push_back(adj[e]);
        }
    if ((int)q.size() != n) return fail(HOMMX_EINVAL, "the mesh is not connected (%d of %d nodes reachable from node 0)", (int)q.size(), n);
  }
  if (d->order) {
    std::vector<char> seen(n, 0);
    for (int k = 0; k < n; ++k) {
      const int v = d->order[k];
      if (v < 0 || v >= n || seen[v]) return fail(HOMMX_EINVAL, "order is not a permutation of [0, %d): entry %d is %d", n, k, v);
      seen[v] = 1;
    }
  }
  // folded node coordinates (the coordinate sweeps of the frontal route, the bisection of the tree route)
  g->y.assign((size_t)n * dim, 0.0);
  for (int e = 0; e < ne; ++e)
    for (int a = 0; a < nv; ++a) {
      const int v = d->el_nodes[e * nv + a];
      for (int c = 0; c < dim; ++c) {
        double q = d->el_x[((size_t)e * nv + a) * dim + c];
        q -= std::floor(q + 1e-9);  // the max faces fold onto the min faces
        g->y[(size_t)v * dim + c] = q;
      }
    }
  return HOMMX_OK;
}

int mesh_geom_upload(const hommx_mesh_desc* d, const MeshGeom& g, MeshGeomDev* out) {
  return upload_packed(&out->block, {{d->el_nodes, sizeof(int32_t) * (size_t)d->n_el * (d->dim + 1), (const void**)&out->el_nodes},
                                     {g.grads.data(), sizeof(double) * g.grads.size(), (const void**)&out->grads},
                                     {g.vol.data(), sizeof(double) * g.vol.size(), (const void**)&out->vol}});
}

int mesh_analyze(const hommx_mesh_desc* d, const MeshGeom& geo, MeshPlan** out, int32_t* front_width, double* flops_per_solve) {
  if (out) *out = nullptr;
  MeshPlan* m = new (std::nothrow) MeshPlan();
  if (!m) return fail(HOMMX_ENOMEM, "host allocation failed");
  struct Guard {
    MeshPlan*& p;
    ~Guard() { delete p; }
  } guard{m};
  const int dim = d->dim, nv = dim + 1;
  const int n = (int)d->n_nodes, ne = (int)d->n_el;
  m->dim = dim;
  m->kind = d->kind;
  const KindSizes ks = kind_sizes(dim, d->kind);
  m->bs = ks.bs;
  m->t = ks.t;
  m->n_comp = ks.n_comp;
  m->n_nodes = n;
  m->n_el = ne;
  const int bs = m->bs, t = m->t;
  const std::vector<int>& ptr = geo.ptr;
  const std::vector<int>& adj = geo.adj;
  if (d->order) {
    m->order.assign(d->order, d->order + n);
  } else {
    // the narrowest of reverse Cuthill-McKee and the coordinate sweeps along every axis
    m->order = rcm_order(n, ptr, adj);
    int best = width_of(m->order, d);
    for (int axis = 0; axis < dim; ++axis) {
      std::vector<int> o = sweep_order(n, dim, geo.y, axis);
      const int w = width_of(o, d);
      if (w < best) {
        best = w;
        m->order.swap(o);
      }
    }
  }
  m->pos.assign(n, 0);
  for (int k = 0; k < n; ++k) m->pos[m->order[k]] = k;
  const int pinned = m->order[n - 1];
  m->n_steps = n - 1;

  // elements by assembly step (the first node of the order they touch), coloured within a step
  std::vector<int> first(ne);
  std::vector<int> cnt(n, 0);
  for (int e = 0; e < ne; ++e) {
    int f = n;
    for (int a = 0; a < nv; ++a) f = std::min(f, m->pos[d->el_nodes[e * nv + a]]);
    first[e] = f;  // < n - 1: an element has at least two distinct nodes
    ++cnt[f];
  }
  std::vector<int> by_step_ptr(n + 1, 0), by_step(ne);
  for (int k = 0; k < n; ++k) by_step_ptr[k + 1] = by_step_ptr[k] + cnt[k];
  {
    std::vector<int> fill(by_step_ptr.begin(), by_step_ptr.end() - 1);
    for (int e = 0; e < ne; ++e) by_step[fill[first[e]]++] = e;
  }
  std::vector<int> slot_of(n, -1), slot_node;  // slot_node[s] = node or -1
  std::vector<int> free_slots;                  // kept sorted descending: back() is the lowest free slot
  int active = 0, hi = 0, width_nodes = 0;
  double flops = 0.0;
  m->step_grp.push_back(0);
  m->grp_ptr.push_back(0);
  std::vector<int> ord_owner;
  for (int k = 0; k < n - 1; ++k) {
    // colour the step's elements greedily: group g holds no two elements with a common node
    std::vector<std::vector<int>> groups;
    std::vector<std::vector<int>> gnodes;
    for (int q = by_step_ptr[k]; q < by_step_ptr[k + 1]; ++q) {
      const int e = by_step[q];
      const int* en = d->el_nodes + (size_t)e * nv;
      size_t g = 0;
      for (; g < groups.size(); ++g) {
        bool clash = false;
        for (int a = 0; a < nv && !clash; ++a)
          clash = std::find(gnodes[g].begin(), gnodes[g].end(), en[a]) != gnodes[g].end();
        if (!clash) break;
      }
      if (g == groups.size()) {
        groups.emplace_back();
        gnodes.emplace_back();
      }
      groups[g].push_back(e);
      gnodes[g].insert(gnodes[g].end(), en, en + nv);
      for (int a = 0; a < nv; ++a) {
        const int v = en[a];
        if (v == pinned || slot_of[v] >= 0) continue;
        int s;
        if (!free_slots.empty()) {
          s = free_slots.back();
          free_slots.pop_back();
        } else {
          s = hi++;
          slot_node.push_back(-1);
        }
        slot_of[v] = s;
        slot_node[s] = v;
        ++active;
      }
    }
    for (auto& g : groups) {
      m->el_seq.insert(m->el_seq.end(), g.begin(), g.end());
      m->grp_ptr.push_back((int)m->el_seq.size());
    }
    m->step_grp.push_back((int)m->grp_ptr.size() - 1);
    const int v = m->order[k];
    width_nodes = std::max(width_nodes, active);
    for (int c = 0; c < bs; ++c) {
      const double f = (double)active * bs - c;
      flops += f * f + 2.0 * f * t;
    }
    m->step_slot.push_back(slot_of[v]);
    m->step_node.push_back(v);
    int top = 0;
    for (int s = 0; s < hi; ++s)
      if (slot_node[s] >= 0) top = s + 1;
    m->step_S.push_back(t + top * bs);
    ord_owner.insert(ord_owner.end(), slot_node.begin(), slot_node.end());
    ord_owner.push_back(-2);  // row separator: hi grows, rows are re-laid out below
    // eliminate: free the slot (lowest free slot first)
    slot_node[slot_of[v]] = -1;
    free_slots.push_back(slot_of[v]);
    std::sort(free_slots.begin(), free_slots.end(), std::greater<int>());
    slot_of[v] = -1;
    --active;
  }
  m->front_width = width_nodes * bs;
  m->flops = flops;
  if (front_width) *front_width = m->front_width;
  if (flops_per_solve) *flops_per_solve = flops;
  if (m->front_width > HOMMX_MESH_MAX_FRONT)
    return fail(HOMMX_EINVAL, "front width %d of the elimination order exceeds HOMMX_MESH_MAX_FRONT = %d (unknowns)", m->front_width,
                 HOMMX_MESH_MAX_FRONT);
  if (!out) return HOMMX_OK;

  m->nslots = hi;
  m->S = t + hi * bs;
  // owner table [n_steps][nslots]
  m->owner.assign((size_t)m->n_steps * hi, -1);
  {
    size_t q = 0;
    for (int k = 0; k < m->n_steps; ++k) {
      int s = 0;
      for (; ord_owner[q] != -2; ++q, ++s) m->owner[(size_t)k * hi + s] = ord_owner[q];
      ++q;
    }
  }
  m->el_slot.assign((size_t)ne * nv, -1);
  for (int e = 0; e < ne; ++e)
    for (int a = 0; a < nv; ++a) {
      // a node keeps its slot for its whole life: the slot it had when the element was assembled
      const int v = d->el_nodes[e * nv + a];
      if (v == pinned) continue;
      const int k = first[e];
      int s = -1;
      for (int j = 0; j < hi && s < 0; ++j)
        if (m->owner[(size_t)k * hi + j] == v) s = j;
      m->el_slot[(size_t)e * nv + a] = s;
    }
  m->piv_off.assign((size_t)m->n_steps * bs + 1, 0);
  for (int k = 0; k < m->n_steps; ++k)
    for (int c = 0; c < bs; ++c) m->piv_off[(size_t)k * bs + c + 1] = m->piv_off[(size_t)k * bs + c] + m->step_S[k];
  // node -> (element, vertex) incidence, CSR; filled element by element, so the entries of a node ascend by element
  m->inc_ptr.assign(n + 1, 0);
  for (size_t q = 0; q < (size_t)ne * nv; ++q) ++m->inc_ptr[d->el_nodes[q] + 1];
  for (int v = 0; v < n; ++v) m->inc_ptr[v + 1] += m->inc_ptr[v];
  m->inc_ent.assign((size_t)ne * nv, 0);
  {
    std::vector<int> fill(m->inc_ptr.begin(), m->inc_ptr.end() - 1);
    for (int e = 0; e < ne; ++e)
      for (int a = 0; a < nv; ++a) m->inc_ent[fill[d->el_nodes[e * nv + a]]++] = (int)((unsigned)e << 2 | (unsigned)a);
  }
  *out = m;
  m = nullptr;  // released from the guard
  return HOMMX_OK;
}

int mesh_upload(MeshPlan* m, const MeshGeomDev& geo) {
  MeshDev& G = m->dev;
  G.grads = geo.grads;
  G.vol = geo.vol;
  if (int rc = upload_packed(&m->d_tables, {{m->el_slot.data(), sizeof(int) * m->el_slot.size(), (const void**)&G.el_slot},
                                            {m->el_seq.data(), sizeof(int) * m->el_seq.size(), (const void**)&G.el_seq},
                                            {m->grp_ptr.data(), sizeof(int) * m->grp_ptr.size(), (const void**)&G.grp_ptr},
                                            {m->step_grp.data(), sizeof(int) * m->step_grp.size(), (const void**)&G.step_grp},
                                            {m->step_slot.data(), sizeof(int) * m->step_slot.size(), (const void**)&G.step_slot},
                                            {m->step_S.data(), sizeof(int) * m->step_S.size(), (const void**)&G.step_S},
                                            {m->piv_off.data(), sizeof(long long) * m->piv_off.size(), (const void**)&G.piv_off},
                                            {m->step_node.data(), sizeof(int) * m->step_node.size(), (const void**)&G.step_node},
                                            {m->owner.data(), sizeof(int) * m->owner.size(), (const void**)&G.owner},
                                            {m->inc_ptr.data(), sizeof(int) * m->inc_ptr.size(), (const void**)&m->inc.ptr},
                                            {m->inc_ent.data(), sizeof(int) * m->inc_ent.size(), (const void**)&m->inc.ent}}))
    return rc;
  m->inc.pinned = m->order.back();
  G.n_el = (int)m->n_el;
  G.n_nodes = (int)m->n_nodes;
  G.n_steps = m->n_steps;
  G.S = m->S;
  char buf[256];
  snprintf(buf, sizeof(buf),
           "mesh_front: k_mesh_front, one workgroup of %d threads per macro cell, packed front of %d rows in LDS (%zu B), %d nodes, %lld "
           "elements, %d assembly groups",
           kThreads, m->S, sizeof(double) * ((size_t)m->S * (m->S + 1) / 2 + m->S + (kThreads / 64) * kRed), (int)m->n_nodes,
           (long long)m->n_el, (int)m->grp_ptr.size() - 1);
  m->detail = buf;
  return HOMMX_OK;
}

void mesh_destroy(MeshPlan* m) {
  if (!m) return;
  if (m->d_tables) (void)hipFree(m->d_tables);
  if (m->d_arena) (void)hipFree(m->d_arena);
  if (m->d_binfo) (void)hipFree(m->d_binfo);
  delete m;
}

int32_t mesh_front_width(const MeshPlan* m) { return m->front_width; }
double mesh_flops_per_cell(const MeshPlan* m) { return m->flops; }
int64_t mesh_num_nodes(const MeshPlan* m) { return m->n_nodes; }
const char* mesh_route_detail(MeshPlan* m) { return m->detail.c_str(); }

namespace {
long long arena_per_cell(const MeshPlan* m) { return (m->piv_off.back() + 31) / 32 * 32; }
// cells per corrector chunk: about 1 GiB of arena, at least one cell
long long arena_chunk(const MeshPlan* m, long long ncells) {
  long long c = (1ll << 27) / std::max(1ll, arena_per_cell(m));
  c = std::max(1ll, std::min(c, 65536ll));
  return std::min(c, ncells);
}
}  // namespace

size_t mesh_arena_bytes_per_cell(const MeshPlan* m) { return sizeof(double) * (size_t)arena_per_cell(m); }
long long mesh_arena_chunk(const MeshPlan* m, long long n_cells) { return arena_chunk(m, n_cells); }

namespace {

template <int DIM, int KIND>
hipError_t launch_front(const MeshPlan* m, long long nc, const double* coef, const double* M, double* out, int32_t* info, double* arena,
                        hipStream_t st) {
  const size_t lds = sizeof(double) * ((size_t)m->S * (m->S + 1) / 2 + m->S + (kThreads / 64) * kRed);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k_mesh_front<DIM, KIND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((k_mesh_front<DIM, KIND>), dim3((unsigned)nc), dim3(kThreads), lds, st, m->dev, coef, M, out, info, arena,
                     arena_per_cell(m));
  return hipGetLastError();
}

hipError_t launch_backsub(const MeshPlan* m, long long nc, const double* arena, const int32_t* info, double* corr, hipStream_t st) {
  const long long apc = arena_per_cell(m);
#define BS_CASE(T, B)                                                                                                 \
  if (m->t == T && m->bs == B) {                                                                                      \
    hipLaunchKernelGGL((k_mesh_backsub<T, B>), dim3((unsigned)nc), dim3(kThreads), 0, st, m->dev, arena, apc, info, corr); \
    return hipGetLastError();                                                                                         \
  }
  BS_CASE(2, 1)
  BS_CASE(3, 1)
  BS_CASE(3, 2)
  BS_CASE(6, 3)
#undef BS_CASE
  return hipErrorInvalidValue;
}
}  // namespace

int mesh_reserve(MeshPlan* m, long long n_cells) {
  (void)m;
  (void)n_cells;
  return HOMMX_OK;  // the effective-tensor path works in LDS only; the corrector arena is sized by the corrector call
}

int mesh_solve(MeshPlan* m, long long ncells, const double* d_coef, const double* d_M, double* d_out, int32_t* d_info, hipStream_t st,
               double* d_corr) {
  if (ncells <= 0) return HOMMX_OK;
  auto front = [&](long long nc, const double* coef, const double* M, double* out, int32_t* info, double* arena) -> hipError_t {
    return dispatch_dim_kind(m->dim, m->kind, [&](auto D, auto K) { return launch_front<D(), K()>(m, nc, coef, M, out, info, arena, st); });
  };
  const int d = m->dim, t = m->t;
  if (!d_corr) {
    for (long long c0 = 0; c0 < ncells; c0 += 0x7fffffffll) {
      const long long nc = std::min(ncells - c0, 0x7fffffffll);
      HIP_TRY(front(nc, d_coef + c0 * m->n_el * m->n_comp, d_M ? d_M + c0 * d * d : nullptr, d_out + c0 * t * t, d_info ? d_info + c0 : nullptr,
                 nullptr));
    }
    return HOMMX_OK;
  }
  const long long chunk = arena_chunk(m, ncells);
  if (chunk > m->cap_arena_cells) {
    if (m->d_arena) (void)hipFree(m->d_arena);
    if (m->d_binfo) (void)hipFree(m->d_binfo);
    m->d_arena = nullptr;
    m->d_binfo = nullptr;
    m->cap_arena_cells = 0;
    HIP_TRY(hipMalloc(&m->d_arena, sizeof(double) * chunk * arena_per_cell(m)));
    HIP_TRY(hipMalloc(&m->d_binfo, sizeof(int32_t) * chunk));
    m->cap_arena_cells = chunk;
  }
  m->arena_valid = chunk == ncells ? ncells : 0;
  const long long nu = m->n_nodes * m->bs;
  for (long long c0 = 0; c0 < ncells; c0 += chunk) {
    const long long nc = std::min(ncells - c0, chunk);
    HIP_TRY(front(nc, d_coef + c0 * m->n_el * m->n_comp, d_M ? d_M + c0 * d * d : nullptr, d_out + c0 * t * t, m->d_binfo, m->d_arena));
    HIP_TRY(launch_backsub(m, nc, m->d_arena, m->d_binfo, d_corr + c0 * t * nu, st));
    if (d_info) HIP_TRY(hipMemcpyAsync(d_info + c0, m->d_binfo, sizeof(int32_t) * nc, hipMemcpyDeviceToDevice, st));
  }
  return HOMMX_OK;
}

int mesh_load_correctors(MeshPlan* m, long long ncells, const LoadOverride& lo, const double* d_M, double* d_corr_l, hipStream_t st) {
  if (ncells <= 0) return HOMMX_OK;
  if (lo.n_loads < 1 || lo.n_loads > m->t || !lo.P) return fail(HOMMX_EINVAL, "load solve: n_loads must be 1 .. %d with loads given", m->t);
  if (ncells > m->arena_valid)
    return fail(HOMMX_EINVAL, "load solve of %lld cells, but the factor arena holds the columns of %lld: the corrector call before it must "
                              "run them as one arena chunk",
                ncells, m->arena_valid);
  HIP_TRY(dispatch_dim_kind(m->dim, m->kind, [&](auto D, auto K) {
    hipLaunchKernelGGL((k_mesh_front_rhs<D(), K()>), dim3((unsigned)ncells), dim3(kThreads), 0, st, m->dev, m->inc, m->d_arena, arena_per_cell(m),
                       m->d_binfo, lo, d_M, d_corr_l);
    return hipGetLastError();
  }));
  return HOMMX_OK;
}

}  // namespace hommx
