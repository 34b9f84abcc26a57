// mesh_tree.h -- internal interface of the tree route of the mesh family (mesh_tree.hip): cell problems on an
// unstructured periodic micro mesh whose frontal width exceeds HOMMX_MESH_MAX_FRONT (or any mesh with HOMMX_MESH_FLAG_TREE), solved by
// the nested-dissection engine of multifrontal.hip.  Only three things are the mesh's own: the tree (recursive coordinate bisection with
// vertex separators), the coupling codes (position of a neighbour in a node's sorted adjacency list) and K1 (k_mesh_assemble).
//
// The symbolic phase is host code: hommx_mesh_analyze_tree and the argument checks of hommx_plan_create_mesh run it without a GPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hommx_hip.h"

namespace hommx {

// device view of the assembly tables (K1 of a mesh plan, launch_mesh_assembly)
struct MeshAsm {
  int dim, kind, nn, n_el, ncode;
  const double* grads;   // [n_el][dim+1][dim]
  const double* vol;     // [n_el]
  const int* cptr;       // [ncode * nn + 1] contributions of (code c, node i) at cptr[c nn + i] .. cptr[c nn + i + 1]
  const int* centry;     // element << 4 | r << 2 | s: local vertex r is node i, s the node of code c; ascending element order
  const int* self_code;  // [nn] code of (i, i)
};

struct MeshTreePlan;

// what hommx_mesh_analyze_tree reports
struct MeshTreeInfo {
  int32_t n_fronts, n_groups, max_front;
  double flops;
};

// Validates the descriptor (mesh_check) and runs the symbolic phase: tree, codes, assembly tables, the host half of the multifrontal plan.
// out == nullptr: analysis only.  supernode_of_node [n_nodes] / parent [n_fronts] may be null.  Errors: mesh_last_error().
int mesh_tree_analyze(const hommx_mesh_desc* d, MeshTreePlan** out, MeshTreeInfo* info, int32_t* supernode_of_node, int32_t* parent);
// device tables and the workspace (the caller has selected the plan's device)
int mesh_tree_upload(MeshTreePlan* m);
void mesh_tree_destroy(MeshTreePlan* m);
double mesh_tree_flops_per_cell(const MeshTreePlan* m);
int64_t mesh_tree_num_nodes(const MeshTreePlan* m);
const char* mesh_tree_route_detail(MeshTreePlan* m);
int mesh_tree_reserve(MeshTreePlan* m, long long n_cells);
// as mesh_solve (mesh_front.h): coef[cell][el][n_comp], M or null -> out[cell][t][t], info; d_corr: correctors [cell][t][n_nodes bs]
int mesh_tree_solve(MeshTreePlan* m, long long ncells, const double* d_coef, const double* d_M, double* d_out, int32_t* d_info,
                    hipStream_t stream, double* d_corr = nullptr);

}  // namespace hommx
