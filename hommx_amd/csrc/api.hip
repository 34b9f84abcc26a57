// api.hip -- the C ABI of libhommx_hip.so (include/hommx_hip.h): plan objects, buffers, dispatch.
//
// Boundary it implements: the macro-cell loop BaseHMM._assemble_stiffness (hmm.py:298-332) calling
// _compute_local_stiffness (hmm.py:334-369) once per cell.  Here: one call per batch of cells.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/hommx_hip.h"
#include "blocked_internal.h"
#include "host_common.h"
#include "kernels.h"
#include "mesh_front.h"
#include "mesh_tree.h"

namespace hommx {

namespace {
thread_local std::string g_err;
}

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int prefix_error(int code, const char* prefix) {
  g_err.insert(0, prefix);
  return code;
}

int upload_packed(void** block, std::initializer_list<HostPiece> pieces) {
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  size_t total = 0;
  for (const HostPiece& p : pieces) total += up(p.bytes);
  std::vector<char> host(total, 0);
  HIP_TRY(hipMalloc(block, total));
  size_t off = 0;
  for (const HostPiece& p : pieces) {
    if (p.bytes) memcpy(host.data() + off, p.src, p.bytes);
    *p.dst = static_cast<const char*>(*block) + off;
    off += up(p.bytes);
  }
  HIP_TRY(hipMemcpy(*block, host.data(), total, hipMemcpyHostToDevice));
  return HOMMX_OK;
}

}  // namespace hommx

namespace {

using hommx::fail;
using hommx::prefix_error;

// FAM_BLOCKED: structured plans beyond the fused 2D kernel, and the mesh plans of the tree route (their workspace carries the mesh)
enum Family { FAM_FUSED2D = 0, FAM_BLOCKED = 1, FAM_MESH = 2 };

// a device (or, pinned, page-locked host) buffer, grown on demand
struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  bool pinned = false;
  void release() {
    if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
};

int grow(Buf& b, size_t bytes) {
  if (bytes <= b.cap) return HOMMX_OK;
  b.release();
  if (b.pinned)
    HIP_TRY(hipHostMalloc(&b.p, bytes, hipHostMallocDefault));
  else
    HIP_TRY(hipMalloc(&b.p, bytes));
  b.cap = bytes;
  return HOMMX_OK;
}

}  // namespace

struct hommx_plan {
  hommx_plan_desc desc;
  Family family;
  int64_t n_el;
  hommx::KindSizes ks;
  hommx::BlockedWorkspace* ws = nullptr;  // FAM_BLOCKED, and a FAM_FUSED2D plan once it has served correctors
  hommx::MeshPlan* mesh = nullptr;        // FAM_MESH: symbolic phase + device tables of the unstructured micro mesh
  // plan-owned staging, grown on demand, never per call: the plain host entry point's buffers, the expanded element stream of the sampler
  // entry points, and the packed blocks of the sampler host entry points (pinned host mirrors + device)
  Buf coef, M, out, info, expand, dev_in, dev_out, pin_in{nullptr, 0, true}, pin_out{nullptr, 0, true};
  // host-pointer entry point: coefficient chunks stream in on s_copy while s_comp solves the previous one
  hipStream_t s_copy = nullptr, s_comp = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  // reconstruction (hommx_reconstruct_batch): HOMMX_RECON_MEM_MB, read when the plan is created; the correctors of one chunk (and the chi^xi
  // slots of cells too large for LDS), A_eff the caller did not ask for, the host entry's staging
  int64_t recon_mem_mb = 1024;
  Buf rcorr, rA, rin, rout;
  // mesh plans: the element table, P1 gradients and volumes on the device, uploaded when the plan is created -- the one copy the route's
  // kernels (MeshDev / MeshAsm) and the reconstruction read
  hommx::MeshGeomDev geo{};
};

namespace {

// what opens a batch entry point, in this order: the plan, the batch size, the pointers (`names` lists them), the limit of one launch (device
// entry points); then the plan's device is made current.  GO, or what the call returns: an error, HOMMX_OK for an empty batch
constexpr int GO = 1;
int open_call(const hommx_plan* p, int64_t n_cells, bool ptrs_ok = true, const char* names = "", bool one_launch = false) {
  if (!p) return fail(HOMMX_EINVAL, "null plan");
  if (n_cells < 0) return fail(HOMMX_EINVAL, "negative n_cells");
  if (n_cells == 0) return HOMMX_OK;
  if (!ptrs_ok) return fail(HOMMX_EINVAL, "null %s", names);
  if (one_launch && n_cells > 0x7fffffffll) return fail(HOMMX_EINVAL, "n_cells too large for one launch");
  HIP_TRY(hipSetDevice(p->desc.device));
  return GO;
}

// HOMMX_RECON_MEM_MB (include/hommx_hip.h): read once, when the plan is created
int64_t recon_mem_mb_env() {
  const char* v = getenv("HOMMX_RECON_MEM_MB");
  const long long mb = v ? atoll(v) : 0;
  return mb > 0 ? mb : 1024;
}

// a failed call into the plan's route, under the route's name
int route_fail(const hommx_plan* p, int rc) { return prefix_error(rc, p->desc.n_micro ? "blocked path: " : "mesh route: "); }

// an element stream on the device through the plan's mesh_front or blocked route; d_corr: the correctors as well
int route_solve(hommx_plan* p, int64_t n_cells, const double* d_coef, const double* d_M, double* d_A_eff, int32_t* d_info, hipStream_t st,
                double* d_corr = nullptr) {
  const int rc = p->family == FAM_MESH ? hommx::mesh_solve(p->mesh, n_cells, d_coef, d_M, d_A_eff, d_info, st, d_corr)
                                       : hommx::blocked_solve(p->ws, n_cells, d_coef, d_M, d_A_eff, d_info, st, d_corr);
  return rc ? route_fail(p, rc) : HOMMX_OK;
}

// a fused 2D plan computes no correctors: the first call that needs them gives it a workspace of the blocked family, which does
int corrector_workspace(hommx_plan* p) {
  if (p->family != FAM_FUSED2D || p->ws) return HOMMX_OK;
  int rc = hommx::blocked_workspace_create(&p->ws, p->desc.dim, p->desc.n_micro, p->desc.kind);
  return rc ? prefix_error(rc, "blocked path: ") : HOMMX_OK;
}

// periodic unknowns of a cell (nodes x bs): the length of one corrector
long long plan_ndof(const hommx_plan* p) { return (p->family == FAM_MESH ? hommx::mesh_num_nodes(p->mesh) : p->ws->G.nn) * (long long)p->ks.bs; }

// the sampler device entry points on the blocked and mesh families: expand(c0, nc, dst) launches the expansion of cells [c0, c0 + nc) into
// the plan's element stream, which is solved chunk by chunk of at most 1 GiB
template <typename Expand>
int expand_and_solve(hommx_plan* p, int64_t n_cells, const double* d_M, double* d_A_eff, int32_t* d_info, hipStream_t st, Expand expand) {
  const int64_t per = p->n_el * p->ks.n_comp;
  const int64_t chunk = std::clamp<int64_t>((1ll << 27) / std::max<int64_t>(per, 1), 1, n_cells);
  if (int rc = grow(p->expand, sizeof(double) * chunk * per)) return rc;
  double* dst = static_cast<double*>(p->expand.p);
  const int d = p->desc.dim, t = p->ks.t;
  for (int64_t c0 = 0; c0 < n_cells; c0 += chunk) {
    const int64_t nc = (n_cells - c0 < chunk) ? n_cells - c0 : chunk;
    HIP_TRY(expand(c0, nc, dst));
    int rc = route_solve(p, nc, dst, d_M ? d_M + c0 * d * d : nullptr, d_A_eff + c0 * t * t, d_info ? d_info + c0 : nullptr, st);
    if (rc != HOMMX_OK) return rc;
  }
  return HOMMX_OK;
}

// The sampler host entry points: their inputs are small, so they are packed into ONE pinned block owned by the plan and travel in one
// asynchronous copy; the outputs come back the same way, and the call synchronises once.  No hipMalloc / hipFree per call.  in[k]: a host
// input (a null one takes no room); run(d_in, d_A_eff, d_info) calls the device entry point with d_in[k] the device copy of in[k] (or null).
struct HostIn {
  const void* src;
  size_t bytes;
};
// the inputs into the plan's pinned block and ONE asynchronous copy to its device twin; d_in[k]: the device copy of in[k] (null for a null input)
template <size_t N>
int stage_in(hommx_plan* p, const HostIn (&in)[N], const void* (&d_in)[N]) {
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  size_t off[N], in_bytes = 0;
  for (size_t k = 0; k < N; ++k) {
    off[k] = in_bytes;
    if (in[k].src) in_bytes += up(in[k].bytes);
  }
  if (int rc = grow(p->pin_in, in_bytes)) return rc;
  if (int rc = grow(p->dev_in, in_bytes)) return rc;
  char* hin = static_cast<char*>(p->pin_in.p);
  char* din = static_cast<char*>(p->dev_in.p);
  for (size_t k = 0; k < N; ++k) {
    d_in[k] = in[k].src ? din + off[k] : nullptr;
    if (in[k].src) memcpy(hin + off[k], in[k].src, in[k].bytes);
  }
  if (in_bytes) HIP_TRY(hipMemcpyAsync(din, hin, in_bytes, hipMemcpyHostToDevice, nullptr));
  return HOMMX_OK;
}

template <size_t N, typename Run>
int staged_call(hommx_plan* p, int64_t n_cells, const HostIn (&in)[N], double* A_eff, int32_t* info, Run run) {
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t a_bytes = sizeof(double) * n_cells * p->ks.t * p->ks.t, o_info = up(a_bytes), out_bytes = o_info + up(sizeof(int32_t) * n_cells);
  if (int rc = grow(p->pin_out, out_bytes)) return rc;
  if (int rc = grow(p->dev_out, out_bytes)) return rc;
  char* dout = static_cast<char*>(p->dev_out.p);
  const void* d_in[N];
  if (int rc = stage_in(p, in, d_in)) return rc;
  if (int rc = run(d_in, reinterpret_cast<double*>(dout), reinterpret_cast<int32_t*>(dout + o_info))) return rc;
  HIP_TRY(hipMemcpyAsync(p->pin_out.p, dout, out_bytes, hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  const char* hout = static_cast<const char*>(p->pin_out.p);
  memcpy(A_eff, hout, a_bytes);
  if (info) memcpy(info, hout + o_info, sizeof(int32_t) * n_cells);
  return HOMMX_OK;
}

// kind and family of a separable sampler (hommx_solve_batch_separable, hommx_reconstruct_source): no device needed
int sampler_check(const hommx_plan* p, int32_t family) {
  if (p->desc.kind != HOMMX_KIND_POISSON_SCALAR && p->desc.kind != HOMMX_KIND_ELASTICITY_ISO)
    return fail(HOMMX_EINVAL, "separable samplers are defined for the scalar Poisson and the isotropic elasticity kinds");
  if (p->desc.kind == HOMMX_KIND_ELASTICITY_ISO && family != HOMMX_SAMPLER_AFFINE)
    return fail(HOMMX_EINVAL, "the isotropic elasticity kind takes the affine sampler only ((lambda, mu) = a + b g)");
  if (family != HOMMX_SAMPLER_AFFINE && family != HOMMX_SAMPLER_RECIPROCAL) return fail(HOMMX_EINVAL, "unknown sampler family %d", family);
  return HOMMX_OK;
}

// the kernels.h form of a separable sampler
hommx::CoefSource sampler_source(int32_t family, int32_t n_q, const double* d_table, const double* d_weights) {
  hommx::CoefSource src;
  src.mode = family == HOMMX_SAMPLER_AFFINE ? hommx::COEF_AFFINE : hommx::COEF_RECIPROCAL;
  src.nq = family == HOMMX_SAMPLER_AFFINE ? 1 : n_q;
  src.table = d_table;
  src.weights = d_weights;
  return src;
}

}  // namespace

extern "C" {

int hommx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* hommx_last_error(void) { return hommx::g_err.c_str(); }

int hommx_plan_create(hommx_plan** out, const hommx_plan_desc* d) {
  if (!out || !d) return fail(HOMMX_EINVAL, "null argument");
  *out = nullptr;
  if (d->dim != 2 && d->dim != 3) return fail(HOMMX_EINVAL, "dim must be 2 or 3 (hmm.py:104-105), got %d", d->dim);
  if (d->kind < 0 || d->kind > 3) return fail(HOMMX_EINVAL, "unknown kind %d", d->kind);
  if (d->n_micro < 3) return fail(HOMMX_EINVAL, "n_micro must be >= 3 (got %d): with fewer cells per side periodic neighbours coincide", d->n_micro);
  int ndev = hommx_device_count();
  if (ndev <= 0) return fail(HOMMX_ENODEV, "no HIP device visible");
  if (d->device < 0 || d->device >= ndev) return fail(HOMMX_EINVAL, "device %d out of range [0,%d)", d->device, ndev);

  hommx_plan* p = new (std::nothrow) hommx_plan();
  if (!p) return fail(HOMMX_ENOMEM, "host allocation failed");
  p->desc = *d;
  p->recon_mem_mb = recon_mem_mb_env();
  const int dim = d->dim, n = d->n_micro;
  p->n_el = (dim == 2) ? 2ll * n * n : 6ll * n * n * n;
  p->ks = hommx::kind_sizes(dim, d->kind);
  const bool fused = dim == 2 && d->kind == HOMMX_KIND_POISSON_SCALAR && n <= 32 && !(d->flags & HOMMX_FLAG_FORCE_BLOCKED);
  p->family = fused ? FAM_FUSED2D : FAM_BLOCKED;
  if (p->family == FAM_BLOCKED) {
    int rc = hommx::blocked_workspace_create(&p->ws, dim, n, d->kind);
    if (rc != 0) {
      delete p;
      return prefix_error(rc, "blocked path: ");
    }
  }
  *out = p;
  return HOMMX_OK;
}

int hommx_plan_destroy(hommx_plan* p) {
  if (!p) return HOMMX_OK;
  hipSetDevice(p->desc.device);
  if (p->ws) hommx::blocked_workspace_destroy(p->ws);
  if (p->mesh) hommx::mesh_destroy(p->mesh);
  for (Buf* b : {&p->coef, &p->M, &p->out, &p->info, &p->expand, &p->dev_in, &p->dev_out, &p->pin_in, &p->pin_out, &p->rcorr, &p->rA, &p->rin,
                 &p->rout})
    b->release();
  if (p->geo.block) (void)hipFree(p->geo.block);
  if (p->s_copy) hipStreamDestroy(p->s_copy);
  if (p->s_comp) hipStreamDestroy(p->s_comp);
  for (hipEvent_t e : p->ev)
    if (e) hipEventDestroy(e);
  delete p;
  return HOMMX_OK;
}

int32_t hommx_plan_dim(const hommx_plan* p) { return p ? p->desc.dim : 0; }
int32_t hommx_plan_device(const hommx_plan* p) { return p ? p->desc.device : -1; }
int32_t hommx_plan_n_micro(const hommx_plan* p) { return p ? p->desc.n_micro : 0; }
int32_t hommx_plan_kind(const hommx_plan* p) { return p ? p->desc.kind : -1; }
int64_t hommx_plan_num_elements(const hommx_plan* p) { return p ? p->n_el : 0; }
int32_t hommx_plan_coef_components(const hommx_plan* p) { return p ? p->ks.n_comp : 0; }
int32_t hommx_plan_tensor_size(const hommx_plan* p) { return p ? p->ks.t : 0; }
int hommx_plan_reserve(hommx_plan* p, int64_t n_cells) {
  if (int rc = open_call(p, n_cells); rc != GO) return rc;
  if (p->family == FAM_FUSED2D) return HOMMX_OK;  // the fused 2D family keeps no scratch
  const int rc = p->family == FAM_MESH ? hommx::mesh_reserve(p->mesh, n_cells) : hommx::blocked_reserve(p->ws, n_cells);
  return rc ? route_fail(p, rc) : HOMMX_OK;
}

double hommx_plan_flops_per_solve(const hommx_plan* p) {
  if (!p) return 0.0;
  switch (p->family) {
    case FAM_FUSED2D: {
      const double n = p->desc.n_micro;
      return (6.0 * (n - 1) + 2.0) * n * n * n;
    }
    case FAM_MESH: return hommx::mesh_flops_per_cell(p->mesh);
    default: return hommx::blocked_flops_per_cell(p->ws);
  }
}

const char* hommx_plan_kernel_name(const hommx_plan* p) {
  if (!p) return "";
  switch (p->family) {
    case FAM_FUSED2D: return "fused2d";
    case FAM_MESH: return "mesh_front";
    default: return hommx::blocked_route_name(p->ws);
  }
}

const char* hommx_plan_route_detail(hommx_plan* p) {
  if (!p) return "";
  switch (p->family) {
    case FAM_FUSED2D:
      return p->desc.n_micro > 16 ? "fused2d: k_poisson2d_fused<32>, one wavefront per macro cell, every matrix in the f64 MFMA accumulator layout"
                                  : "fused2d: k_poisson2d_fused<16>, one wavefront per macro cell, every matrix in the f64 MFMA accumulator layout";
    case FAM_MESH: return hommx::mesh_route_detail(p->mesh);
    default: return hommx::blocked_route_detail(p->ws);
  }
}

int hommx_mesh_analyze(const hommx_mesh_desc* d, int32_t* front_width, double* flops_per_solve) {
  hommx::MeshGeom geo;
  if (int rc = hommx::mesh_check(d, &geo)) return rc;
  return hommx::mesh_analyze(d, geo, nullptr, front_width, flops_per_solve);
}

int hommx_mesh_analyze_tree(const hommx_mesh_desc* d, int32_t* n_fronts, int32_t* n_groups, int32_t* max_front, double* flops_per_solve,
                            int32_t* supernode_of_node, int32_t* parent) {
  hommx::MeshGeom geo;
  if (int rc = hommx::mesh_check(d, &geo)) return rc;
  hommx::MeshTreeInfo info{};
  if (int rc = hommx::mesh_tree_analyze(d, geo, nullptr, &info, supernode_of_node, parent)) return rc;
  if (n_fronts) *n_fronts = info.n_fronts;
  if (n_groups) *n_groups = info.n_groups;
  if (max_front) *max_front = info.max_front;
  if (flops_per_solve) *flops_per_solve = info.flops;
  return HOMMX_OK;
}

int hommx_plan_create_mesh(hommx_plan** out, const hommx_mesh_desc* d) {
  if (!out || !d) return fail(HOMMX_EINVAL, "null argument");
  *out = nullptr;
  // every argument check runs before the device is touched: the mesh is validated once (mesh_check), and both routes analyse that one
  // MeshGeom.  The frontal route takes what fits its LDS front; wider meshes, and any mesh with HOMMX_MESH_FLAG_TREE, take the tree route
  hommx::MeshGeom geo;
  if (int rc = hommx::mesh_check(d, &geo)) return rc;
  hommx::MeshPlan* m = nullptr;
  hommx::MeshTreePlan* mt = nullptr;
  int rc = 0;
  if (!(d->flags & HOMMX_MESH_FLAG_TREE)) {
    int32_t width = 0;
    rc = hommx::mesh_analyze(d, geo, &m, &width, nullptr);
    if (rc && !(rc == HOMMX_EINVAL && width > HOMMX_MESH_MAX_FRONT)) return rc;
  }
  if (!m && (rc = hommx::mesh_tree_analyze(d, geo, &mt, nullptr, nullptr, nullptr)) != 0) return rc;
  auto drop = [&]() {
    hommx::mesh_destroy(m);
    hommx::mesh_tree_destroy(mt);
  };
  int ndev = hommx_device_count();
  if (ndev <= 0 || d->device < 0 || d->device >= ndev) {
    drop();
    return ndev <= 0 ? fail(HOMMX_ENODEV, "no HIP device visible") : fail(HOMMX_EINVAL, "device %d out of range [0,%d)", d->device, ndev);
  }
  hommx_plan* p = new (std::nothrow) hommx_plan();
  if (!p) {
    drop();
    return fail(HOMMX_ENOMEM, "host allocation failed");
  }
  p->desc.dim = d->dim;
  p->desc.n_micro = 0;
  p->desc.kind = d->kind;
  p->desc.device = d->device;
  p->desc.flags = d->flags;
  p->family = m ? FAM_MESH : FAM_BLOCKED;
  p->mesh = m;
  p->n_el = d->n_el;
  p->ks = hommx::kind_sizes(d->dim, d->kind);
  p->recon_mem_mb = recon_mem_mb_env();
  rc = hipSetDevice(d->device) == hipSuccess ? HOMMX_OK : fail(HOMMX_EHIP, "hipSetDevice failed");
  if (!rc) rc = hommx::mesh_geom_upload(d, geo, &p->geo);
  if (!rc) rc = m ? hommx::mesh_upload(m, p->geo) : hommx::mesh_tree_workspace(mt, p->geo, &p->ws);
  hommx::mesh_tree_destroy(mt);  // host analysis only: the workspace holds what the tree route needs
  if (rc) {
    hommx_plan_destroy(p);
    return prefix_error(rc, "mesh route: ");
  }
  *out = p;
  return HOMMX_OK;
}

int32_t hommx_plan_front_width(const hommx_plan* p) { return p && p->family == FAM_MESH ? hommx::mesh_front_width(p->mesh) : 0; }

int hommx_solve_batch_device(hommx_plan* p, int64_t n_cells, const double* d_coef, const double* d_M,
                             double* d_A_eff, int32_t* d_info, void* stream) {
  if (int rc = open_call(p, n_cells, d_coef && d_A_eff, "coef / A_eff", true); rc != GO) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (p->family == FAM_FUSED2D) {
    HIP_TRY(hommx::launch_poisson2d_fused(d_coef, d_M, d_A_eff, d_info, p->desc.n_micro, n_cells, st));
    return HOMMX_OK;
  }
  return route_solve(p, n_cells, d_coef, d_M, d_A_eff, d_info, st);
}

int hommx_solve_batch(hommx_plan* p, int64_t n_cells, const double* coef, const double* M, double* A_eff,
                      int32_t* info) {
  if (int rc = open_call(p, n_cells, coef && A_eff, "coef / A_eff"); rc != GO) return rc;
  const int d = p->desc.dim, t = p->ks.t;
  const int64_t per = p->n_el * p->ks.n_comp;
  if (int rc = grow(p->coef, sizeof(double) * n_cells * per)) return rc;
  if (int rc = grow(p->M, sizeof(double) * n_cells * d * d)) return rc;
  if (int rc = grow(p->out, sizeof(double) * n_cells * t * t)) return rc;
  if (int rc = grow(p->info, sizeof(int32_t) * n_cells)) return rc;
  double* d_coef = static_cast<double*>(p->coef.p);
  double* d_M = M ? static_cast<double*>(p->M.p) : nullptr;
  double* d_out = static_cast<double*>(p->out.p);
  int32_t* d_info = static_cast<int32_t*>(p->info.p);
  if (M) HIP_TRY(hipMemcpy(d_M, M, sizeof(double) * n_cells * d * d, hipMemcpyHostToDevice));
  // cells per chunk of the pipelined copy.  Fused 2D kernel: one wave per cell fills the 256 CUs x 8 wave slots exactly once; blocked
  // family: about 256 MB of coefficient stream, at least 256 cells (from there its throughput is flat: C4 / C5 393 KB per cell -> 682)
  const int64_t CH = p->family == FAM_FUSED2D ? 2048 : std::clamp<int64_t>((256ll << 20) / (8 * std::max<int64_t>(per, 1)), 256, 4096);
  if (n_cells >= 2 * CH) {
    // The coefficient stream (16 KiB per 2D cell, 393 KB per 16^3 elasticity cell) costs PCIe time -- more than the fused kernel costs GPU
    // time, 4 - 8 % of the 3D solves: pipeline it.  The copies are issued from pageable memory, so each blocks this thread -- while the
    // kernels of the previous chunk, already queued on the other stream, run.
    if (!p->s_copy) {
      HIP_TRY(hipStreamCreateWithFlags(&p->s_copy, hipStreamNonBlocking));
      HIP_TRY(hipStreamCreateWithFlags(&p->s_comp, hipStreamNonBlocking));
      HIP_TRY(hipEventCreateWithFlags(&p->ev[0], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&p->ev[1], hipEventDisableTiming));
    }
    int k = 0;
    for (int64_t c0 = 0; c0 < n_cells; c0 += CH, k ^= 1) {
      const int64_t nc = (n_cells - c0 < CH) ? n_cells - c0 : CH;
      HIP_TRY(hipMemcpyAsync(d_coef + c0 * per, coef + c0 * per, sizeof(double) * nc * per, hipMemcpyHostToDevice, p->s_copy));
      HIP_TRY(hipEventRecord(p->ev[k], p->s_copy));
      HIP_TRY(hipStreamWaitEvent(p->s_comp, p->ev[k], 0));
      int rc = hommx_solve_batch_device(p, nc, d_coef + c0 * per, M ? d_M + c0 * d * d : nullptr, d_out + c0 * t * t, d_info + c0, p->s_comp);
      if (rc != HOMMX_OK) return rc;
    }
    HIP_TRY(hipStreamSynchronize(p->s_comp));
  } else {  // batches below two chunks: one copy in front of the kernels
    HIP_TRY(hipMemcpy(d_coef, coef, sizeof(double) * n_cells * per, hipMemcpyHostToDevice));
    int rc = hommx_solve_batch_device(p, n_cells, d_coef, d_M, d_out, d_info, nullptr);
    if (rc != HOMMX_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
  }
  HIP_TRY(hipMemcpy(A_eff, d_out, sizeof(double) * n_cells * t * t, hipMemcpyDeviceToHost));
  if (info) HIP_TRY(hipMemcpy(info, d_info, sizeof(int32_t) * n_cells, hipMemcpyDeviceToHost));
  return HOMMX_OK;
}

int hommx_solve_batch_two_phase_device(hommx_plan* p, int64_t n_cells, const uint8_t* d_mask, const double* d_values,
                                       const double* d_M, double* d_A_eff, int32_t* d_info, void* stream) {
  if (int rc = open_call(p, n_cells, d_mask && d_values && d_A_eff, "mask / values / A_eff", true); rc != GO) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (p->family == FAM_FUSED2D) {
    hommx::CoefSource src;
    src.mode = hommx::COEF_TWO_PHASE;
    src.table = d_mask;
    HIP_TRY(hommx::launch_poisson2d_fused(d_values, d_M, d_A_eff, d_info, p->desc.n_micro, n_cells, st, src));
    return HOMMX_OK;
  }
  const int n_comp = p->ks.n_comp;
  return expand_and_solve(p, n_cells, d_M, d_A_eff, d_info, st, [&](int64_t c0, int64_t nc, double* dst) {
    return hommx::launch_expand_two_phase(d_mask, d_values + c0 * 2 * n_comp, dst, p->n_el, n_comp, nc, st);
  });
}

int hommx_solve_batch_two_phase(hommx_plan* p, int64_t n_cells, const uint8_t* mask, const double* values,
                                const double* M, double* A_eff, int32_t* info) {
  if (int rc = open_call(p, n_cells, mask && values && A_eff, "mask / values / A_eff"); rc != GO) return rc;
  const int d = p->desc.dim;
  const HostIn in[] = {{mask, (size_t)p->n_el}, {values, sizeof(double) * n_cells * 2 * p->ks.n_comp}, {M, sizeof(double) * n_cells * d * d}};
  return staged_call(p, n_cells, in, A_eff, info, [&](const void* const* d_in, double* d_A_eff, int32_t* d_info) {
    return hommx_solve_batch_two_phase_device(p, n_cells, static_cast<const uint8_t*>(d_in[0]), static_cast<const double*>(d_in[1]),
                                              static_cast<const double*>(d_in[2]), d_A_eff, d_info, nullptr);
  });
}

int hommx_solve_batch_separable_device(hommx_plan* p, int64_t n_cells, int32_t family, int32_t n_q, const double* d_table,
                                       const double* d_weights, const double* d_params, const double* d_M, double* d_A_eff,
                                       int32_t* d_info, void* stream) {
  if (int rc = open_call(p, n_cells); rc != GO) return rc;
  if (int rc = sampler_check(p, family)) return rc;
  if (!d_table || !d_params || !d_A_eff) return fail(HOMMX_EINVAL, "null table / params / A_eff");
  if (family == HOMMX_SAMPLER_RECIPROCAL && (n_q < 1 || !d_weights)) return fail(HOMMX_EINVAL, "reciprocal sampler needs n_q >= 1 and weights");
  if (n_cells > 0x7fffffffll) return fail(HOMMX_EINVAL, "n_cells too large for one launch");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const hommx::CoefSource src = sampler_source(family, n_q, d_table, d_weights);
  if (p->family == FAM_FUSED2D) {
    HIP_TRY(hommx::launch_poisson2d_fused(d_params, d_M, d_A_eff, d_info, p->desc.n_micro, n_cells, st, src));
    return HOMMX_OK;
  }
  const int n_comp = p->ks.n_comp;
  return expand_and_solve(p, n_cells, d_M, d_A_eff, d_info, st, [&](int64_t c0, int64_t nc, double* dst) {
    return hommx::launch_expand_separable(src, d_params + 2 * n_comp * c0, dst, p->n_el, n_comp, nc, st);
  });
}

int hommx_solve_batch_separable(hommx_plan* p, int64_t n_cells, int32_t family, int32_t n_q, const double* table,
                                const double* weights, const double* params, const double* M, double* A_eff, int32_t* info) {
  if (int rc = open_call(p, n_cells, table && params && A_eff, "table / params / A_eff"); rc != GO) return rc;
  if (family != HOMMX_SAMPLER_AFFINE && family != HOMMX_SAMPLER_RECIPROCAL) return fail(HOMMX_EINVAL, "unknown sampler family %d", family);
  if (family == HOMMX_SAMPLER_RECIPROCAL && (n_q < 1 || !weights)) return fail(HOMMX_EINVAL, "reciprocal sampler needs n_q >= 1 and weights");
  const int d = p->desc.dim;
  const int64_t ntab = p->n_el * (family == HOMMX_SAMPLER_AFFINE ? 1 : n_q);
  const HostIn in[] = {{table, sizeof(double) * ntab},
                       {n_q > 0 ? weights : nullptr, sizeof(double) * (n_q > 0 ? n_q : 0)},
                       {params, sizeof(double) * n_cells * 2 * p->ks.n_comp},
                       {M, sizeof(double) * n_cells * d * d}};
  return staged_call(p, n_cells, in, A_eff, info, [&](const void* const* d_in, double* d_A_eff, int32_t* d_info) {
    return hommx_solve_batch_separable_device(p, n_cells, family, n_q, static_cast<const double*>(d_in[0]), static_cast<const double*>(d_in[1]),
                                              static_cast<const double*>(d_in[2]), static_cast<const double*>(d_in[3]), d_A_eff, d_info, nullptr);
  });
}

int hommx_solve_batch_correctors(hommx_plan* p, int64_t n_cells, const double* coef, const double* M, double* A_eff,
                                 double* correctors, int32_t* info) {
  if (int rc = open_call(p, n_cells, coef && A_eff && correctors, "coef / A_eff / correctors"); rc != GO) return rc;
  if (int rc = corrector_workspace(p)) return rc;
  const int d = p->desc.dim, t = p->ks.t;
  const long long nn = p->family == FAM_MESH ? hommx::mesh_num_nodes(p->mesh) : p->ws->G.nn;
  // the call's own device buffers, freed when it returns: the correctors can run to gigabytes, the plan keeps none of them
  struct CallBufs {
    Buf coef, M, out, corr, info;
    ~CallBufs() {
      for (Buf* b : {&coef, &M, &out, &corr, &info}) b->release();
    }
  } b;
  const size_t ncoef = sizeof(double) * n_cells * p->n_el * p->ks.n_comp, ncorr = sizeof(double) * n_cells * t * nn * p->ks.bs;
  if (int rc = grow(b.coef, ncoef)) return rc;
  if (int rc = grow(b.out, sizeof(double) * n_cells * t * t)) return rc;
  if (int rc = grow(b.corr, ncorr)) return rc;
  if (int rc = grow(b.info, sizeof(int32_t) * n_cells)) return rc;
  HIP_TRY(hipMemcpy(b.coef.p, coef, ncoef, hipMemcpyHostToDevice));
  if (M) {
    if (int rc = grow(b.M, sizeof(double) * n_cells * d * d)) return rc;
    HIP_TRY(hipMemcpy(b.M.p, M, sizeof(double) * n_cells * d * d, hipMemcpyHostToDevice));
  }
  int rc = route_solve(p, n_cells, static_cast<const double*>(b.coef.p), static_cast<const double*>(b.M.p), static_cast<double*>(b.out.p),
                       static_cast<int32_t*>(b.info.p), nullptr, static_cast<double*>(b.corr.p));
  if (rc != HOMMX_OK) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(A_eff, b.out.p, sizeof(double) * n_cells * t * t, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(correctors, b.corr.p, ncorr, hipMemcpyDeviceToHost));
  if (info) HIP_TRY(hipMemcpy(info, b.info.p, sizeof(int32_t) * n_cells, hipMemcpyDeviceToHost));
  return HOMMX_OK;
}

}  // extern "C"

namespace {

bool recon_in_lds(const hommx_plan* p) { return sizeof(double) * plan_ndof(p) <= hommx::recon_lds_limit(); }

// cells per chunk: HOMMX_RECON_MEM_MB of correctors (with the chi^xi slots of cells too large for LDS) and of `extra` bytes per cell
int64_t recon_chunk(const hommx_plan* p, int64_t n_cells, size_t extra) {
  const long long nd = plan_ndof(p);
  const size_t per = sizeof(double) * nd * (p->ks.t + (recon_in_lds(p) ? 0 : 1)) + extra;
  return std::clamp<int64_t>((int64_t)((p->recon_mem_mb << 20) / per), 1, n_cells);
}

// device pointers of one chunk of a reconstruction
struct ReconIO {
  const double *coef, *M, *xi;
  double *stats, *region_stats, *strain, *flux, *A_eff;
  int32_t* info;
};
// the regions of a call: how many, and the label of every element on the device
struct ReconRegions {
  int32_t n = 0;
  const uint8_t* label = nullptr;
};

// one chunk of at most recon_chunk() cells on the device: the correctors into the plan's scratch, then k_recon
int recon_run(hommx_plan* p, int64_t nc, int64_t chunk, const ReconIO& io, ReconRegions rg, hipStream_t st) {
  const int t = p->ks.t;
  const long long nd = plan_ndof(p);
  const bool lds = recon_in_lds(p);
  if (int rc = grow(p->rcorr, sizeof(double) * chunk * nd * (t + (lds ? 0 : 1)))) return rc;
  double* d_A_eff = io.A_eff;
  if (!d_A_eff) {
    if (int rc = grow(p->rA, sizeof(double) * chunk * t * t)) return rc;
    d_A_eff = static_cast<double*>(p->rA.p);
  }
  double* corr = static_cast<double*>(p->rcorr.p);
  if (int rc = route_solve(p, nc, io.coef, io.M, d_A_eff, io.info, st, corr)) return rc;
  hommx::ReconArgs a;
  a.ndof = nd;
  a.n_el = p->n_el;
  if (p->desc.n_micro) {
    const double n = p->desc.n_micro;
    a.n = p->desc.n_micro;
    a.vol_struct = 1.0 / (p->desc.dim == 2 ? 2.0 * n * n : 6.0 * n * n * n);
  } else {
    a.el_nodes = p->geo.el_nodes;
    a.grads = p->geo.grads;
    a.vol = p->geo.vol;
  }
  a.corr = corr;
  a.coef = io.coef;
  a.M = io.M;
  a.xi = io.xi;
  a.stats = io.stats;
  a.strain = io.strain;
  a.flux = io.flux;
  a.slot = lds ? nullptr : corr + chunk * t * nd;
  a.n_regions = rg.n;
  a.region = rg.label;
  a.region_stats = io.region_stats;
  HIP_TRY(hommx::launch_reconstruct(a, p->desc.dim, p->desc.kind, p->desc.n_micro == 0, nc, st));
  return HOMMX_OK;
}

// the shared argument checks of the reconstruct entry points
int recon_open(hommx_plan* p, int64_t n_cells, const void* coef, const void* xi, const void* stats, const void* strain, const void* flux,
               bool device) {
  if (int rc = open_call(p, n_cells, coef && xi && stats, "coef / xi / stats", device); rc != GO) return rc;
  if (!strain != !flux) return fail(HOMMX_EINVAL, "strain and flux: both or neither");
  if (int rc = corrector_workspace(p)) return rc;  // a reconstruction needs a route that forms correctors
  return GO;
}

// what hommx_reconstruct_source[_device] checks of its source and regions: no device needed, nothing but p->desc read
int source_check(const hommx_plan* p, const hommx_coef_source* s, int32_t n_regions, const void* region, const void* region_stats) {
  if (!s) return fail(HOMMX_EINVAL, "null source");
  switch (s->form) {
    case HOMMX_COEF_SAMPLED:
      if (!s->coef) return fail(HOMMX_EINVAL, "null coef");
      break;
    case HOMMX_COEF_TWO_PHASE:
      if (!s->mask || !s->values) return fail(HOMMX_EINVAL, "null mask / values");
      break;
    case HOMMX_COEF_SEPARABLE:
      if (int rc = sampler_check(p, s->family)) return rc;
      if (!s->table || !s->params) return fail(HOMMX_EINVAL, "null table / params");
      if (s->family == HOMMX_SAMPLER_RECIPROCAL && (s->n_q < 1 || !s->weights))
        return fail(HOMMX_EINVAL, "reciprocal sampler needs n_q >= 1 and weights");
      break;
    default: return fail(HOMMX_EINVAL, "unknown coefficient form %d", s->form);
  }
  if (n_regions < 0 || n_regions > HOMMX_RECON_MAX_REGIONS)
    return fail(HOMMX_EINVAL, "n_regions must be 0 .. %d, got %d", HOMMX_RECON_MAX_REGIONS, n_regions);
  const bool mask_labels = s->form == HOMMX_COEF_TWO_PHASE && n_regions == 2 && !region;
  if (n_regions == 0 ? (region || region_stats) : (!region_stats || (!region && !mask_labels)))
    return fail(HOMMX_EINVAL, "region and region_stats: both with n_regions > 0 (n_regions == 2 of a two-phase source: the mask may be "
                              "the labels), neither with n_regions == 0");
  return HOMMX_OK;
}

// the source with the pointers of its form alone (the others are not the caller's to set)
hommx_coef_source source_of_form(const hommx_coef_source& s) {
  hommx_coef_source o{};
  o.form = s.form;
  if (s.form == HOMMX_COEF_SAMPLED) o.coef = s.coef;
  if (s.form == HOMMX_COEF_TWO_PHASE) o.mask = s.mask, o.values = s.values;
  if (s.form == HOMMX_COEF_SEPARABLE) {
    o.family = s.family;
    o.n_q = s.family == HOMMX_SAMPLER_AFFINE ? 1 : s.n_q;
    o.table = s.table;
    o.weights = s.family == HOMMX_SAMPLER_AFFINE ? nullptr : s.weights;
    o.params = s.params;
  }
  return o;
}
hommx_coef_source sampled_source(const double* coef) {
  hommx_coef_source s{};
  s.form = HOMMX_COEF_SAMPLED;
  s.coef = coef;
  return s;
}

// cells per chunk of a source: recon_chunk() and, for a sampler form, the 1 GiB of expanded element stream (allocated here) of expand_and_solve
int source_chunk(hommx_plan* p, const hommx_coef_source& s, int64_t n_cells, size_t extra, int64_t* chunk) {
  *chunk = recon_chunk(p, n_cells, extra);
  if (s.form == HOMMX_COEF_SAMPLED) return HOMMX_OK;
  const int64_t per = p->n_el * p->ks.n_comp;
  *chunk = std::min(*chunk, std::max<int64_t>((1ll << 27) / std::max<int64_t>(per, 1), 1));
  return grow(p->expand, sizeof(double) * *chunk * per);
}

// The chunk loop of the four reconstruct entry points.  `s` holds device pointers (a sampled stream may still be on the host).  Per chunk
// of cells [c0, c0 + nc): in(c0, nc, io) fills io, bringing in what a host entry stages per chunk; a sampler form is expanded into the
// plan's element stream by the kernels of expand_and_solve; recon_run; out(c0, nc, io) takes the outputs away (host entries).
template <typename In, typename Out>
int recon_chunks(hommx_plan* p, int64_t n_cells, int64_t chunk, const hommx_coef_source& s, ReconRegions rg, hipStream_t st, In in, Out out) {
  const int n_comp = p->ks.n_comp;
  for (int64_t c0 = 0; c0 < n_cells; c0 += chunk) {
    const int64_t nc = std::min(chunk, n_cells - c0);
    ReconIO io{};
    if (int rc = in(c0, nc, io)) return rc;
    if (s.form != HOMMX_COEF_SAMPLED) {
      double* dst = static_cast<double*>(p->expand.p);
      if (s.form == HOMMX_COEF_TWO_PHASE)
        HIP_TRY(hommx::launch_expand_two_phase(s.mask, s.values + c0 * 2 * n_comp, dst, p->n_el, n_comp, nc, st));
      else
        HIP_TRY(hommx::launch_expand_separable(sampler_source(s.family, s.n_q, s.table, s.weights), s.params + c0 * 2 * n_comp, dst, p->n_el,
                                               n_comp, nc, st));
      io.coef = dst;
    }
    if (int rc = recon_run(p, nc, chunk, io, rg, st)) return rc;
    if (int rc = out(c0, nc, io)) return rc;
  }
  return HOMMX_OK;
}

// everything on the device already: the chunks are views of the caller's arrays
int recon_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source& s, const double* d_M, const double* d_xi, ReconRegions rg,
                 double* d_stats, double* d_region_stats, double* d_strain, double* d_flux, double* d_A_eff, int32_t* d_info, hipStream_t st) {
  const int d = p->desc.dim, t = p->ks.t, ns = HOMMX_RECON_NSTATS(t), nr = rg.n * HOMMX_RECON_NREGION(t);
  const int64_t per = p->n_el * p->ks.n_comp;
  int64_t chunk = 0;
  if (int rc = source_chunk(p, s, n_cells, 0, &chunk)) return rc;
  return recon_chunks(
      p, n_cells, chunk, s, rg, st,
      [&](int64_t c0, int64_t, ReconIO& io) {
        const int64_t fo = c0 * p->n_el * t;
        io = ReconIO{s.coef ? s.coef + c0 * per : nullptr,
                     d_M ? d_M + c0 * d * d : nullptr,
                     d_xi + c0 * t,
                     d_stats + c0 * ns,
                     d_region_stats ? d_region_stats + c0 * nr : nullptr,
                     d_strain ? d_strain + fo : nullptr,
                     d_flux ? d_flux + fo : nullptr,
                     d_A_eff ? d_A_eff + c0 * t * t : nullptr,
                     d_info ? d_info + c0 : nullptr};
        return HOMMX_OK;
      },
      [](int64_t, int64_t, const ReconIO&) { return HOMMX_OK; });
}

// host pointers.  What every cell shares (mask, table, weights, labels) and the per-cell values of a sampler form travel once, in the
// plan's pinned block (as staged_call); a sampled stream, M and xi stream in and every output streams out chunk by chunk, so device
// memory is bounded by the chunk
int recon_host(hommx_plan* p, int64_t n_cells, const hommx_coef_source& s, const double* M, const double* xi, int32_t n_regions,
               const uint8_t* region, double* stats, double* region_stats, double* strain, double* flux, double* A_eff, int32_t* info) {
  const int d = p->desc.dim, t = p->ks.t, ns = HOMMX_RECON_NSTATS(t), nr = n_regions * HOMMX_RECON_NREGION(t);
  const bool sampled = s.form == HOMMX_COEF_SAMPLED;
  const int64_t per = p->n_el * p->ks.n_comp, nfield = strain ? 2 * p->n_el * t : 0;
  const size_t nval = sizeof(double) * n_cells * 2 * p->ks.n_comp;
  const HostIn shared[] = {{s.mask, (size_t)p->n_el},  {s.values, nval}, {s.table, sizeof(double) * p->n_el * s.n_q},
                           {s.weights, sizeof(double) * s.n_q}, {s.params, nval}, {region, (size_t)p->n_el}};
  const void* dv[6];
  if (int rc = stage_in(p, shared, dv)) return rc;
  hommx_coef_source ds = s;
  ds.mask = static_cast<const uint8_t*>(dv[0]);
  ds.values = static_cast<const double*>(dv[1]);
  ds.table = static_cast<const double*>(dv[2]);
  ds.weights = static_cast<const double*>(dv[3]);
  ds.params = static_cast<const double*>(dv[4]);
  const ReconRegions rg{n_regions, n_regions ? (region ? static_cast<const uint8_t*>(dv[5]) : ds.mask) : nullptr};
  // per cell, 256-byte aligned blocks: in = [coef | M | xi], out = [stats | A_eff | info | strain | flux | region_stats]
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t in_cell = sizeof(double) * ((sampled ? per : 0) + (M ? d * d : 0) + t);
  const size_t out_cell = sizeof(double) * (ns + nr + t * t + nfield) + sizeof(int32_t);
  int64_t chunk = 0;
  if (int rc = source_chunk(p, s, n_cells, in_cell + out_cell, &chunk)) return rc;
  const size_t o_M = up(sizeof(double) * chunk * (sampled ? per : 0)), o_xi = o_M + (M ? up(sizeof(double) * chunk * d * d) : 0);
  const size_t o_A = up(sizeof(double) * chunk * ns), o_info = o_A + up(sizeof(double) * chunk * t * t);
  const size_t o_strain = o_info + up(sizeof(int32_t) * chunk), o_flux = o_strain + up(sizeof(double) * chunk * p->n_el * t * (strain ? 1 : 0));
  const size_t o_reg = o_flux + up(sizeof(double) * chunk * p->n_el * t * (strain ? 1 : 0));
  if (int rc = grow(p->rin, o_xi + sizeof(double) * chunk * t)) return rc;
  if (int rc = grow(p->rout, o_reg + sizeof(double) * chunk * nr)) return rc;
  char* din = static_cast<char*>(p->rin.p);
  char* dout = static_cast<char*>(p->rout.p);
  double* d_coef = sampled ? reinterpret_cast<double*>(din) : nullptr;
  double* d_M = M ? reinterpret_cast<double*>(din + o_M) : nullptr;
  double* d_xi = reinterpret_cast<double*>(din + o_xi);
  const ReconIO dev{d_coef,
                    d_M,
                    d_xi,
                    reinterpret_cast<double*>(dout),
                    n_regions ? reinterpret_cast<double*>(dout + o_reg) : nullptr,
                    strain ? reinterpret_cast<double*>(dout + o_strain) : nullptr,
                    strain ? reinterpret_cast<double*>(dout + o_flux) : nullptr,
                    reinterpret_cast<double*>(dout + o_A),
                    reinterpret_cast<int32_t*>(dout + o_info)};
  return recon_chunks(
      p, n_cells, chunk, ds, rg, nullptr,
      [&](int64_t c0, int64_t nc, ReconIO& io) {
        if (sampled) HIP_TRY(hipMemcpy(d_coef, s.coef + c0 * per, sizeof(double) * nc * per, hipMemcpyHostToDevice));
        if (M) HIP_TRY(hipMemcpy(d_M, M + c0 * d * d, sizeof(double) * nc * d * d, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_xi, xi + c0 * t, sizeof(double) * nc * t, hipMemcpyHostToDevice));
        io = dev;
        return HOMMX_OK;
      },
      [&](int64_t c0, int64_t nc, const ReconIO& io) {
        HIP_TRY(hipMemcpy(stats + c0 * ns, io.stats, sizeof(double) * nc * ns, hipMemcpyDeviceToHost));
        if (A_eff) HIP_TRY(hipMemcpy(A_eff + c0 * t * t, io.A_eff, sizeof(double) * nc * t * t, hipMemcpyDeviceToHost));
        if (info) HIP_TRY(hipMemcpy(info + c0, io.info, sizeof(int32_t) * nc, hipMemcpyDeviceToHost));
        if (strain) {
          HIP_TRY(hipMemcpy(strain + c0 * p->n_el * t, io.strain, sizeof(double) * nc * p->n_el * t, hipMemcpyDeviceToHost));
          HIP_TRY(hipMemcpy(flux + c0 * p->n_el * t, io.flux, sizeof(double) * nc * p->n_el * t, hipMemcpyDeviceToHost));
        }
        if (n_regions) HIP_TRY(hipMemcpy(region_stats + c0 * nr, io.region_stats, sizeof(double) * nc * nr, hipMemcpyDeviceToHost));
        return HOMMX_OK;
      });
}

}  // namespace

extern "C" {

int hommx_reconstruct_batch_device(hommx_plan* p, int64_t n_cells, const double* d_coef, const double* d_M, const double* d_xi, double* d_stats,
                                   double* d_strain, double* d_flux, double* d_A_eff, int32_t* d_info, void* stream) {
  if (int rc = recon_open(p, n_cells, d_coef, d_xi, d_stats, d_strain, d_flux, true); rc != GO) return rc;
  return recon_device(p, n_cells, sampled_source(d_coef), d_M, d_xi, ReconRegions{}, d_stats, nullptr, d_strain, d_flux, d_A_eff, d_info,
                      reinterpret_cast<hipStream_t>(stream));
}

int hommx_reconstruct_batch(hommx_plan* p, int64_t n_cells, const double* coef, const double* M, const double* xi, double* stats, double* strain,
                            double* flux, double* A_eff, int32_t* info) {
  if (int rc = recon_open(p, n_cells, coef, xi, stats, strain, flux, false); rc != GO) return rc;
  return recon_host(p, n_cells, sampled_source(coef), M, xi, 0, nullptr, stats, nullptr, strain, flux, A_eff, info);
}

int hommx_reconstruct_source_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* d_M, const double* d_xi,
                                    int32_t n_regions, const uint8_t* d_region, double* d_stats, double* d_region_stats, double* d_strain,
                                    double* d_flux, double* d_A_eff, int32_t* d_info, void* stream) {
  // the source and the regions are checked before the plan's device is made current (an empty batch and a null plan are recon_open's)
  if (p && n_cells > 0)
    if (int rc = source_check(p, src, n_regions, d_region, d_region_stats)) return rc;
  if (int rc = recon_open(p, n_cells, src, d_xi, d_stats, d_strain, d_flux, true); rc != GO) return rc;
  const hommx_coef_source s = source_of_form(*src);
  return recon_device(p, n_cells, s, d_M, d_xi, ReconRegions{n_regions, n_regions ? (d_region ? d_region : s.mask) : nullptr}, d_stats,
                      d_region_stats, d_strain, d_flux, d_A_eff, d_info, reinterpret_cast<hipStream_t>(stream));
}

int hommx_reconstruct_source(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* M, const double* xi, int32_t n_regions,
                             const uint8_t* region, double* stats, double* region_stats, double* strain, double* flux, double* A_eff,
                             int32_t* info) {
  if (p && n_cells > 0)
    if (int rc = source_check(p, src, n_regions, region, region_stats)) return rc;
  if (int rc = recon_open(p, n_cells, src, xi, stats, strain, flux, false); rc != GO) return rc;
  return recon_host(p, n_cells, source_of_form(*src), M, xi, n_regions, region, stats, region_stats, strain, flux, A_eff, info);
}

int hommx_calibrate_fp64(int device, double* mfma_flops_per_s, double* fma_flops_per_s) {
  if (!mfma_flops_per_s && !fma_flops_per_s) return fail(HOMMX_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hommx::run_fp64_calibration(mfma_flops_per_s, fma_flops_per_s));
  return HOMMX_OK;
}

int hommx_calibrate_fp64_mfma(int device, double* flops_per_s) { return hommx_calibrate_fp64(device, flops_per_s, nullptr); }
int hommx_calibrate_fp64_detail(int device, double* mfma_flops_per_s, double* fma_flops_per_s, double* mfma_lds_fed_flops_per_s) {
  if (!mfma_flops_per_s && !fma_flops_per_s && !mfma_lds_fed_flops_per_s) return fail(HOMMX_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hommx::run_fp64_calibration(mfma_flops_per_s, fma_flops_per_s, mfma_lds_fed_flops_per_s));
  return HOMMX_OK;
}

}  // extern "C"
