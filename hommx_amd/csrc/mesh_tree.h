// mesh_tree.h -- internal interface of the tree route of the mesh family (mesh_tree.hip): cell problems on an
// unstructured periodic micro mesh whose frontal width exceeds HOMMX_MESH_MAX_FRONT (or any mesh with HOMMX_MESH_FLAG_TREE), solved by
// the nested-dissection engine of multifrontal.hip as a plan of the blocked family.  Only three things are the mesh's own: the tree
// (recursive coordinate bisection with vertex separators), the coupling codes (position of a neighbour in a node's sorted adjacency list)
// and K1 (k_mesh_assemble); the workspace (blocked_workspace_create_mesh) keeps the tree and the assembly tables.
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
  const double* grads;   // [n_el][dim+1][dim]  in the plan's geometry block (MeshGeomDev)
  const double* vol;     // [n_el]
  const int* cptr;       // [ncode * nn + 1] contributions of (code c, node i) at cptr[c nn + i] .. cptr[c nn + i + 1]
  const int* centry;     // element << 4 | r << 2 | s: local vertex r is node i, s the node of code c; ascending element order
  const int* self_code;  // [nn] code of (i, i)
};

// K1 of a mesh plan -- Kst, Brhs and C0 of `nc` cells in the layout launch_assembly (assembly.hip) writes, from the element stream
void launch_mesh_assembly(const MeshAsm& a, const double* coef, const double* Mm, long long nc, hipStream_t st, double* Kst, double* Brhs,
                          double* C0);

struct MeshTreePlan;  // host-side analysis: tree, coupling codes, assembly tables
struct BlockedWorkspace;
struct MeshGeom;     // mesh_front.h
struct MeshGeomDev;

// what hommx_mesh_analyze_tree reports
struct MeshTreeInfo {
  int32_t n_fronts, n_groups, max_front;
  double flops;
};

// The symbolic phase on a checked mesh (mesh_front.h: mesh_check): tree, codes, assembly tables; with `info`, the host half of the
// multifrontal plan as well.  out == nullptr: analysis only.  supernode_of_node [n_nodes] / parent [n_fronts] may be null.
int mesh_tree_analyze(const hommx_mesh_desc* d, const MeshGeom& g, MeshTreePlan** out, MeshTreeInfo* info, int32_t* supernode_of_node,
                      int32_t* parent);
// the plan's workspace of the blocked family on the current device: the assembly tables uploaded, the tree moved in, its multifrontal plan
// built; `m` keeps nothing the workspace needs.  The element geometry stays in the plan's block `geo`
int mesh_tree_workspace(MeshTreePlan* m, const MeshGeomDev& geo, BlockedWorkspace** out);
void mesh_tree_destroy(MeshTreePlan* m);

}  // namespace hommx
