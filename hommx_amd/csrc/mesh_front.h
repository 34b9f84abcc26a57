// mesh_front.h -- internal interface of the mesh route (mesh_front.hip): cell problems on an unstructured periodic micro mesh,
// eliminated by a batched frontal method.
//
// The symbolic phase (validation, elimination order, front slots, assembly groups) is plain host code: hommx_mesh_analyze and the
// argument checks of hommx_plan_create_mesh run it without a GPU.  mesh_upload moves its tables to the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/hommx_hip.h"

namespace hommx {

struct MeshPlan;

// What the routes take from a validated descriptor, made once per plan or analysis call.
struct MeshGeom {
  std::vector<double> grads, vol;  // [n_el][dim+1][dim] P1 gradients, [n_el] volumes (from the unfolded coordinates)
  std::vector<int> ptr, adj;       // node graph: CSR, neighbours sorted ascending, the node itself not included
  std::vector<double> y;           // [n_nodes][dim] node coordinates folded into [0, 1): the max faces fold onto the min faces
};
// The one place a descriptor is validated: every check of hommx_mesh_analyze but the front width.
int mesh_check(const hommx_mesh_desc* d, MeshGeom* g);

// The element geometry of a mesh plan on the device: one block, owned by the plan (api.hip).  The kernel arguments of both routes
// (MeshDev, MeshAsm) and of the derived-output kernels (ElemWalk, kernels.h) point into it.
struct MeshGeomDev {
  void* block;
  const int32_t* el_nodes;  // [n_el][dim+1] the descriptor's element table
  const double* grads;      // [n_el][dim+1][dim]
  const double* vol;        // [n_el]
};
int mesh_geom_upload(const hommx_mesh_desc* d, const MeshGeom& g, MeshGeomDev* out);

// The symbolic phase of the frontal route on a checked mesh.  out == nullptr: analysis only (hommx_mesh_analyze).  Returns 0 or
// HOMMX_EINVAL / HOMMX_ENOMEM.
int mesh_analyze(const hommx_mesh_desc* d, const MeshGeom& g, MeshPlan** out, int32_t* front_width, double* flops_per_solve);
// device tables of the plan (after mesh_analyze with out != nullptr; the caller has selected the plan's device and uploaded the geometry)
int mesh_upload(MeshPlan* m, const MeshGeomDev& geo);
void mesh_destroy(MeshPlan* m);

int32_t mesh_front_width(const MeshPlan* m);
double mesh_flops_per_cell(const MeshPlan* m);
int64_t mesh_num_nodes(const MeshPlan* m);
const char* mesh_route_detail(MeshPlan* m);
// allocate the corrector arena for batches of up to n_cells now (the effective-tensor path keeps no workspace)
int mesh_reserve(MeshPlan* m, long long n_cells);

// coef[cell][el][n_comp] (caller's element order), M[cell][d][d] or null -> out[cell][t][t], info[cell] (may be null);
// d_corr != null: also the correctors [cell][t][n_nodes * bs] (mean-free), by back substitution over the factor arena
int mesh_solve(MeshPlan* m, long long ncells, const double* d_coef, const double* d_M, double* d_out, int32_t* d_info, hipStream_t stream,
               double* d_corr = nullptr);

// Load solves on the factor arena (k_mesh_front_rhs).  A mesh_solve with d_corr leaves the pivot columns of its cells in the plan's arena
// only when it ran them as one arena chunk: callers that follow it with a load solve size their chunks by mesh_arena_bytes_per_cell and
// cap them at mesh_arena_chunk (api.hip, load_chunk).
struct LoadOverride;  // kernels.h
size_t mesh_arena_bytes_per_cell(const MeshPlan* m);
long long mesh_arena_chunk(const MeshPlan* m, long long n_cells);
// The correctors of the loads `lo` of the first ncells cells of the last mesh_solve(..., d_corr) into rows l < n_loads of
// d_corr_l[cell][t][n_nodes * bs] (mean-free; NaN for a cell whose elimination failed; rows l >= n_loads untouched), on `stream`.
// HOMMX_EINVAL when the arena does not hold the columns of that many cells: stale columns are never read.
int mesh_load_correctors(MeshPlan* m, long long ncells, const LoadOverride& lo, const double* d_M, double* d_corr_l, hipStream_t stream);

}  // namespace hommx
