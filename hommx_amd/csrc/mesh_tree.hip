// mesh_tree.hip -- the tree route of the mesh family: an unstructured periodic micro mesh eliminated by the
// nested-dissection engine of multifrontal.hip (staged elimination, gathering Schur updates, the register-resident front kernel, streams,
// the corrector plan and its back substitution), with the three geometric pieces replaced:
//
//   1. the tree: recursive coordinate bisection of the periodic node graph with true VERTEX separators.  A cut in an open direction at
//      the median coordinate takes as separator the nodes below the cut that have a neighbour above it; the first cut in a periodic
//      direction breaks the ring at c and c + 1/2 with two such layers (the wrap layer is the parent of the middle one at the ring cuts
//      the structured builder splits, HOMMX_MF_SPLIT_DEPTH; one front otherwise), after which the direction is open.  No edge joins the
//      two halves once the separator is removed.  Leaves: mf_leaf_max, as on the structured tree.
//   2. the coupling code of (i, j): the position of j in i's sorted adjacency list, i included (at most 127 codes: the tables are int8).
//   3. K1: k_mesh_assemble writes Kst[cell][code(i, j)][a][b][i] = K[(i, a), (j, b)] and the load rows Brhs[cell][m][b][i] by GATHERING the
//      element contributions through a host table in ascending element order (no atomics), k_mesh_c0 sums C0 in a fixed order.  The element
//      formulas are those of the frontal kernel (mesh_elem.h).  A cell's numbers do not depend on where it sits in the batch.
//
// Gauge: the node of highest elimination rank in the root front is pinned (the structured root pins nn - 1 the same way); A_H does not
// depend on it, and correctors come back mean-free per component.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <new>
#include <utility>
#include <vector>

#include "blocked_internal.h"
#include "host_common.h"
#include "kernels.h"
#include "mesh_elem.h"
#include "mesh_front.h"
#include "mesh_tree.h"

namespace hommx {

struct MeshTreePlan {
  Geo G{};
  MfTree tree;
  std::vector<int> cptr, centry, self_code;
};

// ------------------------------------------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------------------------------------------

// One work-item per (cell, slot, node i), the node on the fast lanes (the fast index of Kst): slot c < ncode writes the bs x bs block of
// code c of row node i, slot ncode the t x bs load entries of node i.  Grid-stride: a launch holds fewer than 2^32 work-items.
template <int DIM, int KIND>
__global__ __launch_bounds__(256) void k_mesh_assemble(MeshAsm A, const double* __restrict__ coef, const double* __restrict__ Mall,
                                                       double* __restrict__ Kst, double* __restrict__ Brhs, long long nc) {
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, BS = ks.bs, NCOMP = ks.n_comp;
  constexpr int NV = DIM + 1;
  const int nn = A.nn;
  const long long per_cell = (long long)(A.ncode + 1) * nn;
  const long long total = nc * per_cell;
  for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (long long)gridDim.x * blockDim.x) {
    const long long cell = w / per_cell;
    const long long rem = w - cell * per_cell;
    const int slot = (int)(rem / nn), i = (int)(rem - (long long)slot * nn);
    const double* cc = coef + cell * (long long)A.n_el * NCOMP;
    const double* M = Mall ? Mall + cell * DIM * DIM : nullptr;
    const int list = slot < A.ncode ? slot : A.self_code[i];
    const int q0 = A.cptr[(long long)list * nn + i], q1 = A.cptr[(long long)list * nn + i + 1];
    if (slot < A.ncode) {
      double acc[BS][BS];
#pragma unroll
      for (int a = 0; a < BS; ++a)
#pragma unroll
        for (int b = 0; b < BS; ++b) acc[a][b] = 0.0;
      for (int q = q0; q < q1; ++q) {
        const int ent = A.centry[q], el = ent >> 4, r = (ent >> 2) & 3, s = ent & 3;
        double C[T][T];
        material<DIM, KIND>(cc + (long long)el * NCOMP, C);
        const double vol = A.vol[el];
        const double* gr = A.grads + ((long long)el * NV + r) * DIM;
        const double* gs = A.grads + ((long long)el * NV + s) * DIM;
#pragma unroll
        for (int a = 0; a < BS; ++a) {
          double sa[T], Ca[T];
          strain<DIM, KIND>(gr, M, a, sa);
#pragma unroll
          for (int m = 0; m < T; ++m) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < T; ++k) v += C[m][k] * sa[k];
            Ca[m] = v;
          }
#pragma unroll
          for (int b = 0; b < BS; ++b) {
            double sb[T];
            strain<DIM, KIND>(gs, M, b, sb);
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < T; ++m) v += Ca[m] * sb[m];
            acc[a][b] += vol * v;
          }
        }
      }
      double* Kc = Kst + ((cell * A.ncode + slot) * BS * BS) * (long long)nn + i;
#pragma unroll
      for (int a = 0; a < BS; ++a)
#pragma unroll
        for (int b = 0; b < BS; ++b) Kc[(long long)(a * BS + b) * nn] = acc[a][b];
    } else {  // loads: B[(i, b), m] = -sum_e vol (C s_(r, b))_m over the elements of node i (the self-code list: one entry per element)
      double acc[T][BS];
#pragma unroll
      for (int m = 0; m < T; ++m)
#pragma unroll
        for (int b = 0; b < BS; ++b) acc[m][b] = 0.0;
      for (int q = q0; q < q1; ++q) {
        const int ent = A.centry[q], el = ent >> 4, r = (ent >> 2) & 3;
        double C[T][T];
        material<DIM, KIND>(cc + (long long)el * NCOMP, C);
        const double vol = A.vol[el];
        const double* gr = A.grads + ((long long)el * NV + r) * DIM;
#pragma unroll
        for (int b = 0; b < BS; ++b) {
          double sb[T];
          strain<DIM, KIND>(gr, M, b, sb);
#pragma unroll
          for (int m = 0; m < T; ++m) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < T; ++k) v += C[m][k] * sb[k];
            acc[m][b] -= vol * v;
          }
        }
      }
      double* Bc = Brhs + cell * (long long)T * BS * nn + i;
#pragma unroll
      for (int m = 0; m < T; ++m)
#pragma unroll
        for (int b = 0; b < BS; ++b) Bc[(long long)(m * BS + b) * nn] = acc[m][b];
    }
  }
}

// C0[cell][t][t] = sum_e vol_e C_e: one 256-thread workgroup per cell (grid-stride over cells), element-strided partial sums per thread, a
// butterfly per wave, the four wave totals added in order -- the same summation for every cell wherever it sits in the batch
template <int DIM, int KIND>
__global__ __launch_bounds__(256) void k_mesh_c0(MeshAsm A, const double* __restrict__ coef, double* __restrict__ C0, long long nc) {
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, NCOMP = ks.n_comp;
  constexpr int NTRI = T * (T + 1) / 2;
  __shared__ double red[4][NTRI];
  const int tid = threadIdx.x;
  for (long long cell = blockIdx.x; cell < nc; cell += gridDim.x) {
    const double* cc = coef + cell * (long long)A.n_el * NCOMP;
    double acc[NTRI];
#pragma unroll
    for (int q = 0; q < NTRI; ++q) acc[q] = 0.0;
    for (int el = tid; el < A.n_el; el += 256) {
      double C[T][T];
      material<DIM, KIND>(cc + (long long)el * NCOMP, C);
      const double vol = A.vol[el];
      int q = 0;
#pragma unroll
      for (int m = 0; m < T; ++m)
#pragma unroll
        for (int n = 0; n <= m; ++n, ++q) acc[q] += vol * C[m][n];
    }
#pragma unroll
    for (int q = 0; q < NTRI; ++q) {
      double v = acc[q];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
      if ((tid & 63) == 0) red[tid >> 6][q] = v;
    }
    __syncthreads();
    if (tid < T * T) {
      const int m = tid / T, n = tid % T;
      const int q = m >= n ? m * (m + 1) / 2 + n : n * (n + 1) / 2 + m;
      C0[cell * T * T + tid] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    }
    __syncthreads();
  }
}

void launch_mesh_assembly(const MeshAsm& a, const double* coef, const double* Mm, long long nc, hipStream_t st, double* Kst, double* Brhs,
                          double* C0) {
  const long long work = nc * (long long)(a.ncode + 1) * a.nn;
  const unsigned blocks = (unsigned)std::max(1ll, std::min((work + 255) / 256, 1ll << 20));  // x 256 = 2^28 work-items per launch at most
  const unsigned cblocks = (unsigned)std::max(1ll, std::min(nc, 1ll << 20));
  dispatch_dim_kind(a.dim, a.kind, [&](auto D, auto K) {
    hipLaunchKernelGGL((k_mesh_assemble<D(), K()>), dim3(blocks), dim3(256), 0, st, a, coef, Mm, Kst, Brhs, nc);
    hipLaunchKernelGGL((k_mesh_c0<D(), K()>), dim3(cblocks), dim3(256), 0, st, a, coef, C0, nc);
  });
}

// ------------------------------------------------------------------------------------------------------------------------------
// host side: the tree and the tables
// ------------------------------------------------------------------------------------------------------------------------------

namespace {

struct Bisector {
  int dim, leaf_max, split_depth;
  const std::vector<double>* y;  // [n][dim] folded coordinates
  const std::vector<int>*ptr, *adj;
  std::vector<char> side;        // 0: not in the current selection, 1: below the cut, 2: above
  std::vector<char> sep;         // 1: in a separator of the current split
  MfTree* T;

  int push(std::vector<int> nodes, std::vector<int> ch) {
    T->sn_nodes.push_back(std::move(nodes));
    T->sn_children.push_back(std::move(ch));
    return (int)T->sn_nodes.size() - 1;
  }
  double u(int v, int ax) const { return (*y)[(size_t)v * dim + ax]; }
  // sel: the nodes of the box [lo, hi) (periodic[ax]: the whole ring [0, 1) in that direction); returns its top supernode or -1
  int rec(std::vector<int>& sel, const double* lo, const double* hi, const bool* periodic, int depth) {
    if (sel.empty()) return -1;
    if ((int)sel.size() <= leaf_max) return push(sel, {});
    int ax = 0;
    double ext[3] = {0, 0, 0};
    for (int a = 0; a < dim; ++a) ext[a] = periodic[a] ? 1.0 : hi[a] - lo[a];
    for (int a = 1; a < dim; ++a)
      if (ext[a] > ext[ax]) ax = a;
    double l1[3], h1[3], l2[3], h2[3];
    bool per2[3];
    for (int a = 0; a < 3; ++a) {
      l1[a] = l2[a] = lo[a];
      h1[a] = h2[a] = hi[a];
      per2[a] = periodic[a];
    }
    double cut;
    if (periodic[ax]) {  // a ring: halves [0, 1/2) and [1/2, 1), cut at 1/2 and at the wrap
      cut = 0.5;
      per2[ax] = false;
      l1[ax] = 0.0;
      h1[ax] = 0.5;
      l2[ax] = 0.5;
      h2[ax] = 1.0;
    } else {  // the median coordinate
      std::vector<double> c(sel.size());
      for (size_t k = 0; k < sel.size(); ++k) c[k] = u(sel[k], ax);
      std::nth_element(c.begin(), c.begin() + c.size() / 2, c.end());
      cut = c[c.size() / 2];
      h1[ax] = cut;
      l2[ax] = cut;
    }
    for (int v : sel) side[v] = u(v, ax) < cut ? 1 : 2;
    // separators: an edge across the middle cut takes its lower node, an edge across the wrap (periodic only) its upper node
    std::vector<int> sepMid, sepWrap;
    for (int v : sel) {
      if (side[v] != 1) continue;
      const double uv = u(v, ax);
      for (int e = (*ptr)[v]; e < (*ptr)[v + 1]; ++e) {
        const int w = (*adj)[e];
        if (side[w] != 2) continue;
        if (!periodic[ax] || u(w, ax) - uv < 0.5) {
          if (!sep[v]) {
            sep[v] = 1;
            sepMid.push_back(v);
          }
        } else if (!sep[w]) {
          sep[w] = 1;
          sepWrap.push_back(w);
        }
      }
    }
    std::vector<int> a_, b_;
    for (int v : sel)
      if (!sep[v]) (side[v] == 1 ? a_ : b_).push_back(v);
    if (sepMid.empty() && sepWrap.empty()) {  // the halves do not touch: one node of the lower half stands in as the (trivial) separator
      std::vector<int>& from = a_.empty() ? b_ : a_;
      sepMid.push_back(from.back());
      from.pop_back();
    }
    for (int v : sel) side[v] = sep[v] = 0;
    if (a_.empty() && b_.empty()) return push(sel, {});
    sel.clear();
    sel.shrink_to_fit();
    const int ca = rec(a_, l1, h1, per2, depth + 1);
    const int cb = rec(b_, l2, h2, per2, depth + 1);
    std::vector<int> kids;
    if (ca >= 0) kids.push_back(ca);
    if (cb >= 0) kids.push_back(cb);
    // as TreeBuilder::rec: the two layers of a ring cut form a chain of two fronts (middle below the wrap) only at depth <= split_depth
    if (!sepWrap.empty() && !sepMid.empty() && depth <= split_depth) {
      const int mid = push(sepMid, kids);
      return push(sepWrap, {mid});
    }
    sepWrap.insert(sepWrap.end(), sepMid.begin(), sepMid.end());
    return push(sepWrap, kids);
  }
};

}  // namespace

int mesh_tree_analyze(const hommx_mesh_desc* d, const MeshGeom& geo, MeshTreePlan** out, MeshTreeInfo* info, int32_t* supernode_of_node,
                      int32_t* parent) {
  if (out) *out = nullptr;
  const int dim = d->dim, nv = dim + 1;
  const int n = (int)d->n_nodes, ne = (int)d->n_el;
  if (ne >= (1 << 27)) return fail(HOMMX_EINVAL, "the tree route takes fewer than 2^27 elements, got %d", ne);
  std::unique_ptr<MeshTreePlan> m(new (std::nothrow) MeshTreePlan());
  if (!m) return fail(HOMMX_ENOMEM, "host allocation failed");
  const KindSizes ks = kind_sizes(dim, d->kind);
  const int bs = ks.bs;

  // coupling codes: position in the sorted list {i} u adj(i)
  std::vector<int> lptr(n + 1, 0), lst;
  lst.reserve(geo.adj.size() + n);
  int ncode = 0;
  for (int v = 0; v < n; ++v) {
    const int b0 = (int)lst.size();
    lst.insert(lst.end(), geo.adj.begin() + geo.ptr[v], geo.adj.begin() + geo.ptr[v + 1]);
    lst.insert(std::lower_bound(lst.begin() + b0, lst.end(), v), v);
    lptr[v + 1] = (int)lst.size();
    ncode = std::max(ncode, lptr[v + 1] - lptr[v]);
  }
  if (ncode > 127) {
    int worst = 0;
    for (int v = 0; v < n; ++v)
      if (lptr[v + 1] - lptr[v] == ncode) worst = v;
    return fail(HOMMX_EINVAL,
                "node %d couples with %d other nodes: the tree route's coupling codes are int8 (at most 127 per node, itself included)", worst,
                ncode - 1);
  }
  auto code_of = [&](int i, int j) { return (int)(std::lower_bound(lst.begin() + lptr[i], lst.begin() + lptr[i + 1], j) - (lst.begin() + lptr[i])); };

  // the tree
  {
    Bisector B;
    B.dim = dim;
    B.leaf_max = mf_leaf_max(dim, bs);
    B.split_depth = mf_split_depth();
    B.y = &geo.y;
    B.ptr = &geo.ptr;
    B.adj = &geo.adj;
    B.side.assign(n, 0);
    B.sep.assign(n, 0);
    B.T = &m->tree;
    std::vector<int> all(n);
    for (int v = 0; v < n; ++v) all[v] = v;
    const double lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
    const bool per[3] = {true, true, true};
    B.rec(all, lo, hi, per, 0);
  }
  MfTree& T = m->tree;
  // couplings for the plan: node w coupled with v, and the code of (row w, column v)
  T.nb_ptr = lptr;
  T.nb_node = lst;
  T.nb_code.resize(lst.size());
  for (int v = 0; v < n; ++v)
    for (int e = lptr[v]; e < lptr[v + 1]; ++e) T.nb_code[e] = code_of(lst[e], v);

  Geo& G = m->G;
  G.dim = dim;
  G.n = 0;
  G.bs = bs;
  G.t = ks.t;
  G.kind = d->kind;
  G.ncomp = ks.n_comp;
  G.nn = n;
  G.ncode = ncode;
  G.n_el = ne;

  const int nsn = (int)T.sn_nodes.size();
  if (supernode_of_node)
    for (int k = 0; k < nsn; ++k)
      for (int v : T.sn_nodes[k]) supernode_of_node[v] = k;
  if (parent) {
    for (int k = 0; k < nsn; ++k) parent[k] = -1;
    for (int k = 0; k < nsn; ++k)
      for (int c : T.sn_children[k]) parent[c] = k;
  }
  if (info) {  // the host half of the plan mesh_tree_workspace builds
    MfPlan* P = nullptr;
    if (int rc = mf_plan_build(&P, G, T, false)) return rc;
    const MfStats s = mf_stats(P);
    mf_plan_destroy(P);
    info->n_fronts = s.nfronts;
    info->n_groups = s.ngroups;
    info->max_front = s.max_front;
    info->flops = s.flops;
  }
  if (!out) return HOMMX_OK;

  // assembly tables: the contributions of every (code, node), element by element
  {
    const int nslot = ncode * n;
    std::vector<int> cnt(nslot + 1, 0);
    for (int e = 0; e < ne; ++e)
      for (int r = 0; r < nv; ++r)
        for (int s = 0; s < nv; ++s) {
          const int i = d->el_nodes[e * nv + r], j = d->el_nodes[e * nv + s];
          ++cnt[code_of(i, j) * n + i + 1];
        }
    for (int k = 0; k < nslot; ++k) cnt[k + 1] += cnt[k];
    m->cptr = cnt;
    m->centry.assign((size_t)cnt[nslot], 0);
    std::vector<int> fill(cnt.begin(), cnt.end() - 1);
    for (int e = 0; e < ne; ++e)
      for (int r = 0; r < nv; ++r)
        for (int s = 0; s < nv; ++s) {
          const int i = d->el_nodes[e * nv + r], j = d->el_nodes[e * nv + s];
          m->centry[fill[code_of(i, j) * n + i]++] = e << 4 | r << 2 | s;
        }
    m->self_code.resize(n);
    for (int v = 0; v < n; ++v) m->self_code[v] = code_of(v, v);
  }
  *out = m.release();
  return HOMMX_OK;
}

int mesh_tree_workspace(MeshTreePlan* m, const MeshGeomDev& geo, BlockedWorkspace** out) {
  *out = nullptr;
  MeshAsm A{m->G.dim, m->G.kind, m->G.nn, m->G.n_el, m->G.ncode, geo.grads, geo.vol};
  void* tables = nullptr;
  if (int rc = upload_packed(&tables, {{m->cptr.data(), sizeof(int) * m->cptr.size(), (const void**)&A.cptr},
                                       {m->centry.data(), sizeof(int) * m->centry.size(), (const void**)&A.centry},
                                       {m->self_code.data(), sizeof(int) * m->self_code.size(), (const void**)&A.self_code}})) {
    (void)hipFree(tables);
    return rc;
  }
  return blocked_workspace_create_mesh(out, m->G, std::move(m->tree), A, tables);
}

void mesh_tree_destroy(MeshTreePlan* m) { delete m; }

}  // namespace hommx
