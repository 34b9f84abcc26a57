// blocked_internal.h -- everything the translation units of the blocked family share: the workspace object behind a plan and its route
// (blocked.hip), K1 (assembly.hip), the batched fp64-MFMA building blocks both eliminations are made of (dense.hip: GEMM tiles, recursive
// block inverse), the block-cyclic plane elimination (plane.hip), nested dissection (multifrontal.hip) and the one-launch kernels for small
// plane blocks (small.hip, small_wave.hip).  What api.hip calls is declared in kernels.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include "geo.h"
#include "kernels.h"
#include "mesh_tree.h"

namespace hommx {

struct MfPlan;  // multifrontal.hip

// Symbolic input of a nested-dissection plan, from either source (the box dissection of the n^d torus, or the coordinate bisection of an
// unstructured mesh: mesh_tree.hip): the supernode tree and the coupling graph.  Nothing in it is geometric.
struct MfTree {
  std::vector<std::vector<int>> sn_nodes;     // nodes of every supernode; children come before their parent, the root is the last
  std::vector<std::vector<int>> sn_children;  // at most two per supernode (MfChild has two slots)
  std::vector<int> nb_ptr, nb_node, nb_code;  // CSR over nodes v: every node w coupled with v (v included) and the code of (row w, column v)
};

// What a plan launches for effective tensors, decided once when its workspace is created (blocked.hip: ws_configure)
enum class Route { SmallWave, SmallFused, Plane, Tree, MeshTree };

// Buffers of the plane elimination (plane.hip), `chunk` / `hchunk` cells each: one device block per set.  The one-launch kernels take K1
// from here as well.
struct PlaneBufs {
  long long chunk = 0;
  void* block = nullptr;
  double *Kst = nullptr, *Brhs = nullptr, *C0 = nullptr;
  double* Cn = nullptr;        // magnitude normalisation: the scaled coefficient stream of the chunk
  double* EshSlot = nullptr;   // its exponents: carved from the block like the others (one 8-byte slot per cell), read through esh()
  int32_t* esh() const { return reinterpret_cast<int32_t*>(EshSlot); }
  double *S = nullptr, *W = nullptr, *Sl = nullptr, *V = nullptr, *X = nullptr, *T = nullptr;
  double *R = nullptr, *Rl = nullptr, *Vr = nullptr, *Gm = nullptr;
  // corrector mode: per eliminated plane the inverse Schur block, the arrow block and the load rows are kept
  long long hchunk = 0;
  void* hblock = nullptr;
  double *hS = nullptr, *hW = nullptr, *hR = nullptr, *Xa = nullptr, *Xb = nullptr, *Y = nullptr;
};

struct BlockedWorkspace {
  Geo G;
  Route route = Route::Plane;
  int small_nw = 0;            // Route::SmallFused: waves per macro cell (HOMMX_SMALL_WAVES, or the default of the padded block)
  // development knobs, read ONCE when the plan is created (include/hommx_hip.h lists them)
  double budget_gb_env = 0.0;  // HOMMX_BLOCKED_MEM_GB (0: automatic)
  int gemm128_min = 256;       // HOMMX_GEMM128_MIN
  PlaneBufs plane;
  // nested-dissection route (large plane blocks, and every mesh plan of the tree route): the tree both plans are built from (mf_plan_from_tree)
  MfTree tree;
  MfPlan* mf = nullptr;
  MfPlan* mf_keep = nullptr;   // corrector plan of the same route (fronts keep their factors), created by the first corrector call
  bool mf_corr = true;         // HOMMX_MF_CORR=0: correctors of structured multifrontal plans take the plane elimination (A/B runs)
  bool tree_loads = false;     // load solves substitute on the kept fronts of mf_keep (blocked_enable_tree_loads; only where correctors stay on the tree)
  // mesh plans of the tree route (blocked_workspace_create_mesh): K1 is the mesh assembly on these tables, one device block owned here
  MeshAsm mesh{};
  void* mesh_tables = nullptr;  // non-null marks a mesh workspace
  // tile orders of big lower-triangle updates (gemm): device tables, one per tile count, made on first use
  int tile_sb = 4;                // HOMMX_TILE_SB: tiles walk the lower triangle in SB x SB super-blocks (0: row by row)
  std::map<int, int*> tilemaps;
  std::string detail;             // hommx_plan_route_detail: written once, on first request
};

inline unsigned nblk(long long work, int bs = 256) { return (unsigned)((work + bs - 1) / bs); }

// One batched operation context: `nc` matrices (cells, or cells x fronts of one shape) on stream `st`.
struct Ctx {
  BlockedWorkspace* ws;
  long long nc;
  hipStream_t st;
  int32_t* info;          // per CELL failure flags (nullable)
  int stepcode;           // value a failing pivot check writes into info
  int ld = 0;             // leading dimension of the matrices invert() works on (0: G.Bp)
  long long sS = 0;       // their batch stride (0: Bp * Bp)
  long long sT = 0;       // batch stride of invert()'s scratch (0: sS)
  int infoDiv = 1;        // info index = batch index / infoDiv (fronts per cell in the multifrontal route)
};

// Child slot of a multifrontal front (multifrontal.hip), as the kernels see it
struct MfChild {
  long long offF;           // per-cell arena offset (doubles) of the child's GROUP buffer (x chunk size at launch)
  int nf, fidx, L, sp;      // fronts in the child's group, the child's index in it, its leading dimension, its padded s
  int valid, rb;            // rb: first border row of the child's boundary block
};

// "C is virtual": instead of beta * C the GEMM epilogue adds, for every child slot, the child's update matrix entry the unknown pair maps
// to (the extend-add of the multifrontal method fused into the parent's Schur update).  batch b = cell * nf + front.
struct GatherC {
  const double* arena = nullptr;
  long long nc = 0;             // cells in the chunk (arena offsets are per cell)
  const MfChild* child = nullptr;   // [nf][2]
  const int32_t* dpos = nullptr;    // [nf][2][rp] unknown of the child's boundary block a boundary unknown of this front maps to, -1: none
  int nf = 0, rp = 0;
  long long batch0 = 0;         // batch index of matrix 0 of this launch (a huge batch is launched in pieces)
  int rowOff = 0;               // C row 0 is boundary unknown rowOff of the front (the border rows are updated by a launch of their own)
};

// C = alpha op(A) op(B) + beta C for every matrix of the batch (dense.hip: k_gemm_tile, XCD-aware tiles); lowerOnly: tiles on and
// below the diagonal only; Ct: mirrored copy of the result (may be C itself with lowerOnly)
void gemm(const Ctx& c, bool ta, bool tb, int M, int N, int K, double alpha, const double* A, int lda, long long sA, const double* B,
          int ldb, long long sB, double beta, double* C, int ldc, long long sC, int lowerOnly = 0, double* Ct = nullptr,
          const GatherC* gather = nullptr);

// tile edge (64 or 128) gemm() uses for an M x N x K product of this workspace, and the super-block tile order of a lower triangle of `ty`
// tile rows (device table cached in the workspace; nullptr: row-by-row order)
int gemm_tile_size(const BlockedWorkspace* ws, int M, int N, int K, bool gather);
const int* ensure_tilemap(BlockedWorkspace* ws, int ty);

// in-place inverse of the SPD diagonal block [off, off + size) of every matrix of the batch (recursive Schur-complement form;
// size a multiple of 32); `tmp`: scratch of at least size^2 / 2 doubles per matrix, batch stride c.sT
void invert(const Ctx& c, double* S, int off, int size, double* tmp);

// supernode tree of the n^d torus (TreeBuilder: two planes per periodic direction, one per open one) with its stencil couplings
void mf_tree_structured(const Geo& G, MfTree* T);
// leaf size and ring-split depth of both tree builders (HOMMX_MF_LEAF, HOMMX_MF_SPLIT_DEPTH)
int mf_leaf_max(int dim, int bs);
int mf_split_depth();

// multifrontal.hip: the plan of ws->tree on the current device (keep: the corrector plan, every front keeps its factors)
int mf_plan_from_tree(BlockedWorkspace* ws, bool keep, MfPlan** out);
// its host half on any tree: boundaries, heights, groups, arena, flop model and the index tables (no GPU); the gauge is the node of highest
// elimination rank in the root.  G supplies nn, bs, ncode.  loads (with keep): the row block of mf_load_correctors is sized as well.
int mf_plan_build(MfPlan** out, const Geo& G, const MfTree& T, bool keep, bool loads = false);
// what the host analysis found: fronts, groups, the largest front (s + r, unknowns), the largest (s, r) pair, arena doubles per cell, groups on
// k_mf_front
struct MfStats {
  int nfronts, ngroups, max_front, max_s, max_r, front_groups;
  long long arena_per_cell;
  double flops;
};
MfStats mf_stats(const MfPlan* p);
void mf_plan_destroy(MfPlan* p);
double mf_flops_per_cell(const MfPlan* p);
std::string mf_describe(const BlockedWorkspace* ws, const MfPlan* p);  // one line: tree, stages, streams, tile sizes of the dense kernels
int mf_reserve(BlockedWorkspace* ws, MfPlan* P, long long ncells, bool ahead);
// effective tensors, and with the corrector plan (keep = true) and d_corr != nullptr the correctors [cell][t][n^d bs] as well
int mf_solve(BlockedWorkspace* ws, MfPlan* P, long long ncells, const double* d_coef, const double* d_M, double* d_out, int32_t* d_info,
             hipStream_t st, double* d_corr = nullptr, const LoadOverride* loads = nullptr);
// The correctors of the loads `lo` of the nc cells whose factors the last corrector solve of the corrector plan P (of a workspace with
// tree_loads) left in its arena: forward substitution up the tree on a row block of all fronts, then mf_solve's back substitution and
// centring.  HOMMX_EINVAL unless that solve ran exactly these nc cells as one chunk (its halves and streams are taken over)
int mf_load_correctors(BlockedWorkspace* ws, MfPlan* P, long long nc, const LoadOverride& lo, const double* d_M, double* d_corr_l, hipStream_t st);
long long mf_chunk(const MfPlan* P);  // cells per chunk of the plan's buffers (0 before the first reservation)
// loads.hip: Brhs of `nc` cells (the layout K1 writes) from the loads of cells [cell0, cell0 + nc) of `lo`, on the geometry of the workspace
hipError_t launch_assemble_loads(const BlockedWorkspace* ws, const LoadOverride& lo, long long cell0, const double* Mm, long long nc,
                                 hipStream_t st, double* Brhs);
// remove the mean of every component of nc x t corrector fields (blocked.hip)
void launch_center_corr(BlockedWorkspace* ws, double* corr, long long nc, hipStream_t st);
// workspace of a mesh plan of the tree route (mesh_tree_workspace): G (nn = n_nodes, ncode = most coupling codes of a node, n unused), the
// tree, and the assembly tables on the device, which the workspace owns from here on (also on failure); the same development knobs as
// blocked_workspace_create
int blocked_workspace_create_mesh(BlockedWorkspace** out, const Geo& G, MfTree&& tree, const MeshAsm& a, void* tables);
// assembly.hip: corner offsets and P1 gradients of the sub-elements of a structured cell (Geo::voff, Geo::grad)
void fill_tables(Geo& G);
// K1 of the blocked family (stencil rows, loads, C0 of `nc` cells into the given buffers), shared by both eliminations: each route owns
// its buffers (a plan may serve effective tensors on one route and correctors on the other, with different chunk sizes)
void launch_assembly(BlockedWorkspace* ws, const double* coef, const double* Mm, long long nc, hipStream_t st, double* Kst, double* Brhs,
                     double* C0);

// assembly.hip: magnitude normalisation of the blocked family.  The exchange sweeps of the one-launch kernels and of the tree's
// leaves (sweep_acc.h) lose eps |d| on a pivot |d| >> 1, so every route eliminates a cell whose coefficient is scaled by a power of two
// 2^-esh[cell] that brings the stiffness diagonal to order one: `scaled` = coef * 2^-esh is what K1 reads, and the tensors are scaled back
// by launch_scale_cells(out, t t, esh, +1).  Exact, and the correctors do not see it; user-supplied loads (launch_assemble_loads) are scaled
// with launch_scale_cells(Brhs, ., esh, -1) so that their correctors do not either.  NaN / Inf / all-zero cells take esh = 0.
void launch_coef_normalise(const Geo& G, const double* coef, const double* Mm, long long nc, hipStream_t st, double* scaled, int32_t* esh);
void launch_scale_cells(double* buf, long long per_cell, const int32_t* esh, int sign, long long nc, hipStream_t st);

// plane.hip: buffers for batches of up to `ncells` (chunked by the memory budget), with the history set when correctors are asked for
int plane_reserve(BlockedWorkspace* ws, long long ncells, bool correctors);
void plane_free(BlockedWorkspace* ws);
// K2 and K3 of the c.nc cells whose K1 is in ws->plane: tensors to `out`, and with corr != nullptr the correctors [cell][t][n^d bs]
int plane_eliminate(Ctx c, double* out, double* corr);

// small.hip: LDS-resident elimination of a Route::SmallFused plan (small_fused.h), nw = 2, 4 or 8 waves per macro cell
hipError_t launch_small_fused(const Geo& G, const double* Kst, const double* Brhs, const double* C0, double* out, int32_t* info,
                              long long ncells, int nw, hipStream_t stream);
// small_wave.hip: register-resident elimination of a Route::SmallWave plan, one wavefront per macro cell (small_wave.h)
hipError_t launch_small_wave(const Geo& G, const double* Kst, const double* Brhs, const double* C0, double* out, int32_t* info,
                             long long ncells, hipStream_t stream);

}  // namespace hommx
