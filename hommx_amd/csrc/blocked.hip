// blocked.hip -- the workspace behind a plan of the blocked family: any dimension (2, 3), any problem kind (scalar / matrix-valued
// Poisson, isotropic / general elasticity), optional stratification matrix M, any n_micro >= 3; meshes through mesh_tree.hip.
// Created once per plan: the development knobs are read, the route is decided (ws_configure), and every blocked_* entry point switches
// on that decision.  K1 is in assembly.hip (mesh plans: mesh_front.hip), the eliminations in small_wave.hip / small.hip (one launch),
// plane.hip (block-cyclic over node planes) and multifrontal.hip (nested dissection); K3 is  A_H = C0 - G  (== the energy functional
// hmm.py:652-667 / 774-789 / 905-922 / 1050-1067).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>

#include "../../include/hommx_hip.h"
#define HOMMX_HIP_TRY_FMT "%s: %s"
#include "blocked_internal.h"
#include "host_common.h"
#include "kernels.h"

namespace hommx {

// remove the mean of every component (the reference projects the constants out: cell_problem.py:349-361, 382)
__global__ __launch_bounds__(256) void k_center_corr(Geo G, double* __restrict__ corr) {
  __shared__ double red[256];
  double* x = corr + (long long)blockIdx.x * G.nn * G.bs;  // one (cell, load case) per block
  for (int al = 0; al < G.bs; ++al) {
    double acc = 0.0;
    for (int p = threadIdx.x; p < G.nn; p += 256) acc += x[(long long)p * G.bs + al];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
      __syncthreads();
    }
    const double mean = red[0] / G.nn;
    __syncthreads();
    for (int p = threadIdx.x; p < G.nn; p += 256) x[(long long)p * G.bs + al] -= mean;
  }
}

void launch_center_corr(BlockedWorkspace* ws, double* corr, long long nc, hipStream_t st) {
  hipLaunchKernelGGL(k_center_corr, dim3((unsigned)(nc * ws->G.t)), dim3(256), 0, st, ws->G, corr);
}

// the nested-dissection routes, and whether corrector solves stay on them (a mesh has no planes to take)
static bool ws_on_tree(const BlockedWorkspace* ws) { return ws->route == Route::Tree || ws->route == Route::MeshTree; }
static bool ws_corr_on_tree(const BlockedWorkspace* ws) { return ws->route == Route::MeshTree || (ws->route == Route::Tree && ws->mf_corr); }

// Development knobs of a workspace (include/hommx_hip.h), read once when it is created, and the route they and the plane block select.
// Nested dissection (multifrontal.hip) wherever it beats the plane elimination (profiles/r03_kinds_routes.txt) -- every plane
// block b > 64, i.e. everything the one-launch kernels do not take: 2D scalar n = 80: +51 %, 2D elasticity n = 36: +92 %, 3D elasticity
// n = 5: +68 %, n = 16: +76 %, scalar 3D n = 9: +18 % (it lost 10 % there before the build kernel batched its loads and the route ran on
// two streams)
// Round 4: with the register-resident front kernel (mf_front_kernel.h: one launch per tree level, fronts never leave the registers) the tree
// also beats the LDS kernel of csrc/small_fused.h on 2D meshes with 48 < b <= 64: 2D Poisson 64^2 175 k -> 256 k solves/s, 2D elasticity
// 32^2 320 k -> 336 k; it loses on 3D Poisson 8^3 (1.25 M -> 0.79 M: few, larger fronts) and against the one-wave kernel (b <= 48).
static void ws_configure(BlockedWorkspace* ws) {
  const Geo& G = ws->G;
  if (const char* e = getenv("HOMMX_BLOCKED_MEM_GB")) ws->budget_gb_env = atof(e);
  const char* gemm128 = getenv("HOMMX_GEMM128_MIN");
  if (gemm128) ws->gemm128_min = atoi(gemm128);
  if (const char* e = getenv("HOMMX_MF_CORR")) ws->mf_corr = atoi(e) != 0;
  if (const char* e = getenv("HOMMX_TILE_SB")) ws->tile_sb = atoi(e);
  const bool small_fused = getenv("HOMMX_NO_SMALL_FUSED") == nullptr;  // off: no one-launch kernels (A/B runs)
  const char* sw_env = getenv("HOMMX_SMALL_WAVES");  // 2 / 4 (b > 48: 8 as well): the LDS kernel with that many waves per macro cell
  const int sw = sw_env ? atoi(sw_env) : 0;
  // smallest plane block b routed to the tree (0: never); a threshold from the environment below 65 takes effect only together with
  // HOMMX_NO_SMALL_FUSED (A/B runs)
  const char* mf_env = getenv("HOMMX_MF_MIN_B");
  const int mf_min_b = mf_env ? atoi(mf_env) : G.dim == 2 ? 49 : 65;
  if (ws->mesh_tables) ws->route = Route::MeshTree;
  else if (mf_min_b > 0 && G.b >= mf_min_b && (G.b > 64 || !small_fused || (!mf_env && G.b > 48))) ws->route = Route::Tree;
  else if (G.b <= 64 && small_fused) {
    // the whole elimination in ONE launch -- b <= 48: one wave per macro cell, matrices in registers (small_wave.h); 48 < b <= 64, or
    // HOMMX_SMALL_WAVES = 2 | 4: that many waves per cell, matrices in LDS (small_fused.h; 64: 8 waves (two tiles each) +3..5 % over 4)
    ws->route = (G.b <= 48 && sw != 2 && sw != 4) ? Route::SmallWave : Route::SmallFused;
    ws->small_nw = (sw == 2 || sw == 4 || sw == 8) ? sw : 8;
  } else ws->route = Route::Plane;
  // the products of the tree routes are tall and thin or lower-triangular: with the super-block tile order the 64 x 64 tiles (six workgroups
  // per CU) are never slower than the 128 x 128 ones any more -- C4 +2 %, 3D elasticity 20^3 +2 %, scalar 24^3 -1.5 %
  if (ws_on_tree(ws) && !gemm128) ws->gemm128_min = 1 << 30;
}

// knobs and route of a workspace whose G (and mesh) is set and, on the tree routes, the plan; a workspace that fails is destroyed
static int ws_finish(BlockedWorkspace* ws, BlockedWorkspace** out) {
  ws_configure(ws);
  if (ws->route == Route::Tree) mf_tree_structured(ws->G, &ws->tree);
  if (ws_on_tree(ws))
    if (int rc = mf_plan_from_tree(ws, false, &ws->mf)) {
      blocked_workspace_destroy(ws);
      return rc;
    }
  *out = ws;
  return 0;
}

int blocked_workspace_create(BlockedWorkspace** out, int dim, int n, int kind) {
  *out = nullptr;
  BlockedWorkspace* ws = new BlockedWorkspace();
  Geo& G = ws->G;
  const KindSizes ks = kind_sizes(dim, kind);
  G.dim = dim;
  G.n = n;
  G.kind = kind;
  G.bs = ks.bs;
  G.t = ks.t;
  G.ncomp = ks.n_comp;
  G.nn = dim == 2 ? n * n : n * n * n;
  G.npl = dim == 2 ? n : n * n;
  G.b = G.bs * G.npl;
  G.Bp = (G.b + 31) / 32 * 32;
  G.nsub = dim == 2 ? 2 : 6;
  G.ncode = dim == 2 ? 9 : 27;
  G.n_el = G.nsub * G.nn;
  fill_tables(G);
  return ws_finish(ws, out);
}

int blocked_workspace_create_mesh(BlockedWorkspace** out, const Geo& G, MfTree&& tree, const MeshAsm& a, void* tables) {
  *out = nullptr;
  BlockedWorkspace* ws = new BlockedWorkspace();
  ws->G = G;
  ws->tree = std::move(tree);
  ws->mesh = a;
  ws->mesh_tables = tables;
  return ws_finish(ws, out);
}

const char* blocked_route_name(const BlockedWorkspace* ws) {
  static const char* const names[] = {"small_wave", "small_fused", "blocked", "multifrontal", "mesh_multifrontal"};  // in the order of Route
  return ws ? names[(int)ws->route] : "blocked";
}

const char* blocked_corrector_route_name(const BlockedWorkspace* ws) { return ws && ws_corr_on_tree(ws) ? blocked_route_name(ws) : "blocked"; }

// Load solves on the kept fronts of the corrector plan (multifrontal.hip: mf_load_correctors).  Asked for before the corrector plan exists
// (it sizes the row block of the forward pass); a workspace whose correctors do not stay on the tree ignores the request
void blocked_enable_tree_loads(BlockedWorkspace* ws) {
  if (ws && !ws->mf_keep) ws->tree_loads = ws_corr_on_tree(ws);
}

bool blocked_tree_loads(const BlockedWorkspace* ws) { return ws && ws->tree_loads; }

const char* blocked_load_route_name(const BlockedWorkspace* ws) {
  if (!blocked_tree_loads(ws)) return blocked_corrector_route_name(ws);
  return ws->route == Route::MeshTree ? "mesh_multifrontal_subst" : "multifrontal_subst";
}

// the corrector plan of a tree route, created by the first call that needs it
static int ws_keep_plan(BlockedWorkspace* ws) { return ws->mf_keep ? 0 : mf_plan_from_tree(ws, true, &ws->mf_keep); }

long long blocked_tree_load_chunk(BlockedWorkspace* ws, long long n_cells) {
  if (!blocked_tree_loads(ws) || n_cells <= 0) return 0;
  if (ws_keep_plan(ws) || mf_reserve(ws, ws->mf_keep, n_cells, false)) return 0;
  return mf_chunk(ws->mf_keep);
}

int blocked_load_correctors(BlockedWorkspace* ws, long long nc, const LoadOverride& lo, const double* d_M, double* d_corr_l, hipStream_t st) {
  if (!blocked_tree_loads(ws) || !ws->mf_keep)
    return fail(HOMMX_EINVAL, "%s: no corrector solve has left fronts to substitute on", blocked_load_route_name(ws));
  return mf_load_correctors(ws, ws->mf_keep, nc, lo, d_M, d_corr_l, st);
}

// one line for reports (bench.py's roofline.kernel): what the route launches, derived from the plan itself
const char* blocked_route_detail(BlockedWorkspace* ws) {
  if (!ws) return "";
  if (ws->detail.empty()) {
    char buf[512];
    const Geo& G = ws->G;
    if (ws->route == Route::MeshTree) {
      const MfStats s = mf_stats(ws->mf);
      snprintf(buf, sizeof(buf),
               "mesh_multifrontal: coordinate bisection of %lld nodes, %d fronts in %d groups (largest s = %d, r = %d unknowns), arena %.1f MB per "
               "cell, %d group(s) on k_mf_front, %d coupling codes; K1 k_mesh_assemble + k_mesh_c0; ",
               (long long)G.nn, s.nfronts, s.ngroups, s.max_s, s.max_r, 8e-6 * s.arena_per_cell, s.front_groups, G.ncode);
      ws->detail = std::string(buf) + mf_describe(ws, ws->mf);
    } else if (ws->route == Route::Tree)
      ws->detail = mf_describe(ws, ws->mf);
    else if (ws->route == Route::Plane) {
      snprintf(buf, sizeof(buf), "blocked: plane elimination, b = %d (padded %d), k_gemm_tile %s f64-MFMA tiles, recursive block inverse on 32 / 64 leaves, strip-form sparse products",
               G.b, G.Bp, G.Bp >= ws->gemm128_min ? "128x128 (8 waves) and 64x64 (4 waves)" : "64x64 (4 waves)");
      ws->detail = buf;
    } else {
      snprintf(buf, sizeof(buf), "%s: one launch after K1 (k_assemble_reg), plane block b = %d, f64 MFMA 16x16x4 tiles in %s", blocked_route_name(ws), G.b,
               ws->route == Route::SmallWave ? "registers (one wavefront per macro cell)" : "LDS (several waves per macro cell)");
      ws->detail = buf;
    }
  }
  return ws->detail.c_str();
}

double blocked_flops_per_cell(const BlockedWorkspace* ws) {
  if (!ws) return 0.0;
  if (ws_on_tree(ws)) return mf_flops_per_cell(ws->mf);
  const double b = ws->G.b;
  return (6.0 * (ws->G.n - 1) + 2.0) * b * b * b;
}

void blocked_workspace_destroy(BlockedWorkspace* ws) {
  if (!ws) return;
  if (ws->mf) mf_plan_destroy(ws->mf);
  if (ws->mf_keep) mf_plan_destroy(ws->mf_keep);
  if (ws->mesh_tables) (void)hipFree(ws->mesh_tables);
  for (auto& kv : ws->tilemaps) (void)hipFree(kv.second);
  plane_free(ws);
  delete ws;
}

int blocked_reserve(BlockedWorkspace* ws, long long n_cells) {
  if (!ws || n_cells <= 0) return 0;
  if (ws_on_tree(ws)) return mf_reserve(ws, ws->mf, n_cells, true);
  return plane_reserve(ws, n_cells, false);
}

int blocked_solve(BlockedWorkspace* ws, long long ncells, const double* d_coef, const double* d_M, double* d_out,
                  int32_t* d_info, hipStream_t st, double* d_corr, const LoadOverride* loads) {
  if (loads && !d_corr) return fail(HOMMX_EINVAL, "blocked_solve: a load override needs the correctors");
  if (ws_on_tree(ws) && !d_corr) return mf_solve(ws, ws->mf, ncells, d_coef, d_M, d_out, d_info, st);  // nested dissection (multifrontal.hip)
  // correctors on the same route: a second plan whose fronts keep their factors for the back substitution
  if (ws_corr_on_tree(ws)) {
    if (int rc = ws_keep_plan(ws)) return rc;
    return mf_solve(ws, ws->mf_keep, ncells, d_coef, d_M, d_out, d_info, st, d_corr, loads);
  }
  if (int rc = plane_reserve(ws, ncells, d_corr != nullptr)) return rc;
  const Geo& G = ws->G;
  const PlaneBufs& pb = ws->plane;
  if (d_info) HIP_TRY(hipMemsetAsync(d_info, 0, sizeof(int32_t) * ncells, st));
  long long step_cells = d_corr ? std::min(pb.chunk, pb.hchunk) : pb.chunk;
  if (step_cells > 0) {  // equal chunks: a short tail chunk would run the small kernels of the inverse underfilled
    const long long nchunks = (ncells + step_cells - 1) / step_cells;
    step_cells = (ncells + nchunks - 1) / nchunks;
  }
  for (long long c0 = 0; c0 < ncells; c0 += step_cells) {
    const long long nc = std::min(step_cells, ncells - c0);
    Ctx c{ws, nc, st, d_info ? d_info + c0 : nullptr, 0};
    const double* coef = d_coef + c0 * G.n_el * G.ncomp;
    const double* Mm = d_M ? d_M + c0 * G.dim * G.dim : nullptr;
    double* out = d_out + c0 * G.t * G.t;
    // K1 reads the cell at magnitude one (blocked_internal.h, launch_coef_normalise); the tensors go back to the caller's magnitude below
    int32_t* esh = pb.esh();
    launch_coef_normalise(G, coef, Mm, nc, st, pb.Cn, esh);
    launch_assembly(ws, pb.Cn, Mm, nc, st, pb.Kst, pb.Brhs, pb.C0);
    if (loads) {
      HIP_TRY(launch_assemble_loads(ws, *loads, c0, Mm, nc, st, pb.Brhs));
      launch_scale_cells(pb.Brhs, (long long)G.t * G.bs * G.nn, esh, -1, nc, st);
    }
    if (d_corr || ws->route == Route::Plane) {
      if (int rc = plane_eliminate(c, out, d_corr ? d_corr + c0 * (long long)G.t * G.nn * G.bs : nullptr)) return rc;
    } else if (ws->route == Route::SmallWave) HIP_TRY(launch_small_wave(G, pb.Kst, pb.Brhs, pb.C0, out, c.info, nc, st));
    else HIP_TRY(launch_small_fused(G, pb.Kst, pb.Brhs, pb.C0, out, c.info, nc, ws->small_nw, st));
    launch_scale_cells(out, (long long)G.t * G.t, esh, +1, nc, st);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

}  // namespace hommx
