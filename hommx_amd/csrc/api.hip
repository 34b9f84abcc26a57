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
#include "coef_program.h"
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
  std::vector<size_t> bytes, off(pieces.size());
  for (const HostPiece& p : pieces) bytes.push_back(p.bytes);
  const size_t total = pack_offsets(bytes.size(), bytes.data(), off.data());
  std::vector<char> host(total, 0);
  HIP_TRY(hipMalloc(block, total));
  size_t k = 0;
  for (const HostPiece& p : pieces) {
    if (p.bytes) memcpy(host.data() + off[k], p.src, p.bytes);
    *p.dst = static_cast<const char*>(*block) + off[k++];
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

// `b` grown to one block of pieces of bytes[k] bytes (host_common.h, pack_offsets); at[k]: where piece k starts, null for an empty piece;
// *total: the size of the block
template <size_t N>
int carve(Buf& b, const size_t (&bytes)[N], char* (&at)[N], size_t* total = nullptr) {
  size_t off[N];
  const size_t all = hommx::pack_offsets(N, bytes, off);
  if (total) *total = all;
  if (int rc = grow(b, all)) return rc;
  for (size_t k = 0; k < N; ++k) at[k] = bytes[k] ? static_cast<char*>(b.p) + off[k] : nullptr;
  return HOMMX_OK;
}

// The plan-owned buffers, grown on demand, never per call.  B_IN / B_OUT: the device block of the per-cell inputs / outputs of a host
// entry point (hommx_solve_batch: the batch; derived_call: one chunk).  B_EXPAND: the expanded element stream of the sampler forms.
// B_PIN_* / B_DEV_*: the small inputs of the sampler host entry points and their outputs, pinned host mirrors + device (plan_new pins).
// B_RCORR, B_RA: the correctors of one reconstruction chunk (and the chi^xi slots of cells too large for LDS), A_eff the caller did not ask for
// B_FACT: the factor records of one chunk of a fused 2D plan's corrector route (kernels.h)
// B_LOADS: what a load pass leaves where a corrector pass leaves A_eff (hommx_loads_source: C0 - f^T K^+ f, unused)
// B_REFINE: canonical flux field and correction of the refinement step of a fused 2D plan's correctors (10 n^2 doubles per cell)
// B_SENS2: the polarisation loads of one direction of a second-derivative chunk (t n_el t doubles per cell)
// B_TANGENT: the tangents of one chunk of a program source, one stream per differentiable slot (its parameters, then its fields):
//            [nc][n_params + n_fields][n_el][n_comp] (grown with B_EXPAND, by stream_chunk)
// B_CURVATURE: the second-order streams of such a chunk, one per pair a <= b of the slots, [nc][n_pairs][n_el][n_comp], and behind
//            them, at [chunk][n_pairs][n_el][n_comp], the first derivatives of A_H along them, [nc][n_pairs][t][t] (stream_chunk too)
// B_POLAR: the loads of one chunk of hommx_loads_source that the device forms: the expansion of a program load, [nc][n_el][t]
//            (derived_call; an eigenstrain becomes the eigenstress in place), or the eigenstresses of an eigenstrain array that is not
//            the plan's to overwrite, [nc][n_loads][n_el][t] (loads_run; crit_run: the one load of a criterion)
// B_SECANT: the current and the candidate element stream of one chunk of hommx_secant_source, [chunk][n_el][n_comp] each, the info
//            of its eliminations where the caller takes none, [chunk], and the tangent stream of a chunk of hommx_secant_tangent_source
//            where the caller takes none, [chunk][n_el][t (t + 1) / 2], and beside an eigenstrain (hommx_secant_load_source) the
//            eigenstress of the round, [chunk][n_el][t] (secant_run)
// B_REGION: the element labels of the reconstruction tail of the host entry hommx_secant_state_source, [n_el] bytes, uploaded once per call
enum {
  B_IN, B_OUT, B_EXPAND, B_PIN_IN, B_DEV_IN, B_PIN_OUT, B_DEV_OUT, B_RCORR, B_RA, B_FACT, B_LOADS, B_REFINE, B_SENS2, B_TANGENT, B_CURVATURE,
  B_POLAR, B_SECANT, B_REGION, N_BUF
};

}  // namespace

struct hommx_plan {
  hommx_plan_desc desc;
  Family family;
  int64_t n_el;
  hommx::KindSizes ks;
  hommx::BlockedWorkspace* ws = nullptr;  // FAM_BLOCKED, and a FAM_FUSED2D plan with HOMMX_FUSED_CORR=0 once it has served correctors
  bool fused_corr = true;                 // FAM_FUSED2D: correctors by substitution on the fused kernel's own factors (HOMMX_FUSED_CORR)
  bool fused_loads = true;                // ... and the correctors of user loads on the same records (HOMMX_FUSED_LOADS; needs fused_corr)
  hommx::MeshPlan* mesh = nullptr;        // FAM_MESH: symbolic phase + device tables of the unstructured micro mesh
  Buf buf[N_BUF];
  // host-pointer entry point: coefficient chunks stream in on s_copy while s_comp solves the previous one
  hipStream_t s_copy = nullptr, s_comp = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  // reconstruction (hommx_reconstruct_batch): HOMMX_RECON_MEM_MB, read when the plan is created
  int64_t recon_mem_mb = 1024;
  // mesh plans: the element table, P1 gradients and volumes on the device, uploaded when the plan is created -- the one copy the route's
  // kernels (MeshDev / MeshAsm) and the reconstruction read
  hommx::MeshGeomDev geo{};
};

namespace {

// what opens a batch entry point, in this order: the plan, the batch size, the entry's own checks of a non-empty batch (`more`: a
// coefficient source, regions), the pointers (`names` lists them), the limit of one launch (device entry points).  Nothing but p->desc
// is read.  Only then is the plan's device made current.  GO, or what the call
// returns: an error, HOMMX_OK for an empty batch
constexpr int GO = 1;
int one_launch_check(int64_t n_cells) {
  return n_cells > 0x7fffffffll ? fail(HOMMX_EINVAL, "n_cells too large for one launch") : HOMMX_OK;
}
template <typename More>
int open_call(const hommx_plan* p, int64_t n_cells, bool ptrs_ok, const char* names, bool one_launch, More more) {
  if (!p) return fail(HOMMX_EINVAL, "null plan");
  if (n_cells < 0) return fail(HOMMX_EINVAL, "negative n_cells");
  if (n_cells == 0) return HOMMX_OK;
  if (int rc = more()) return rc;
  if (!ptrs_ok) return fail(HOMMX_EINVAL, "null %s", names);
  if (one_launch)
    if (int rc = one_launch_check(n_cells)) return rc;
  HIP_TRY(hipSetDevice(p->desc.device));
  return GO;
}
int open_call(const hommx_plan* p, int64_t n_cells, bool ptrs_ok = true, const char* names = "", bool one_launch = false) {
  return open_call(p, n_cells, ptrs_ok, names, one_launch, [] { return HOMMX_OK; });
}

// What both plan constructors end with: the device range, then the plan with everything its descriptor determines.
// HOMMX_RECON_MEM_MB, HOMMX_FUSED_CORR and HOMMX_FUSED_LOADS (include/hommx_hip.h) are read here, once
int plan_new(hommx_plan** out, const hommx_plan_desc& desc, int64_t n_el) {
  const int ndev = hommx_device_count();
  if (ndev <= 0) return fail(HOMMX_ENODEV, "no HIP device visible");
  if (desc.device < 0 || desc.device >= ndev) return fail(HOMMX_EINVAL, "device %d out of range [0,%d)", desc.device, ndev);
  hommx_plan* p = new (std::nothrow) hommx_plan();
  if (!p) return fail(HOMMX_ENOMEM, "host allocation failed");
  p->desc = desc;
  p->n_el = n_el;
  p->ks = hommx::kind_sizes(desc.dim, desc.kind);
  p->buf[B_PIN_IN].pinned = p->buf[B_PIN_OUT].pinned = true;
  const char* v = getenv("HOMMX_RECON_MEM_MB");
  const long long mb = v ? atoll(v) : 0;
  p->recon_mem_mb = mb > 0 ? mb : 1024;
  if (const char* e = getenv("HOMMX_FUSED_CORR")) p->fused_corr = atoi(e) != 0;
  if (const char* e = getenv("HOMMX_FUSED_LOADS")) p->fused_loads = atoi(e) != 0;
  *out = p;
  return HOMMX_OK;
}

// a fused 2D plan whose correctors come from its own factors
bool fused_subst(const hommx_plan* p) { return p->family == FAM_FUSED2D && p->fused_corr; }
// ... and whose load solve substitutes on the same records (k_fused2d_subst_rhs) instead of eliminating once more on the blocked route
bool fused_loads(const hommx_plan* p) { return fused_subst(p) && p->fused_loads; }
// a frontal mesh plan created with HOMMX_MESH_FLAG_LOADS: its load solve substitutes on the pivot columns of the corrector arena
// (k_mesh_front_rhs)
bool mesh_loads(const hommx_plan* p) { return p->family == FAM_MESH && (p->desc.flags & HOMMX_MESH_FLAG_LOADS) != 0; }
// a plan of a nested-dissection route created with HOMMX_FLAG_TREE_LOADS / HOMMX_MESH_FLAG_TREE_LOADS whose correctors stay on the tree:
// its load solve substitutes on the fronts the canonical pass of the chunk has left in the corrector plan's arena (mf_load_correctors)
bool tree_loads(const hommx_plan* p) { return p->family == FAM_BLOCKED && hommx::blocked_tree_loads(p->ws); }
// bytes of factor record per cell of that route (0 on every other)
size_t fact_bytes(const hommx_plan* p) { return fused_subst(p) ? sizeof(double) * hommx::fused_fact_doubles(p->desc.n_micro) : 0; }
// ... and of the scratch of its refinement step: the canonical flux field (8 n^2 doubles) and the correction (2 n^2)
size_t refine_bytes(const hommx_plan* p) { return fused_subst(p) ? sizeof(double) * 10 * p->desc.n_micro * p->desc.n_micro : 0; }

// a failed call into the plan's route, under the route's name
int route_fail(const hommx_plan* p, int rc) { return prefix_error(rc, p->desc.n_micro ? "blocked path: " : "mesh route: "); }

// an element stream on the device through the plan's mesh_front or blocked route; d_corr: the correctors as well
int route_solve(hommx_plan* p, int64_t n_cells, const double* d_coef, const double* d_M, double* d_A_eff, int32_t* d_info, hipStream_t st,
                double* d_corr = nullptr) {
  if (d_corr && fused_subst(p)) {
    // the fused elimination once more, keeping its block inverses, then the substitution on them: A_eff and info from the forward kernel
    if (int rc = grow(p->buf[B_FACT], fact_bytes(p) * n_cells)) return rc;
    double* fact = static_cast<double*>(p->buf[B_FACT].p);
    HIP_TRY(hommx::launch_poisson2d_fused_fact(d_coef, d_M, d_A_eff, d_info, p->desc.n_micro, n_cells, st, fact));
    HIP_TRY(hommx::launch_fused2d_subst(fact, d_corr, p->desc.n_micro, n_cells, st));
    // one refinement step: the substitution on explicit block inverses loses a larger multiple of cond(K) eps than a sparse LU
    const size_t nn = (size_t)p->desc.n_micro * p->desc.n_micro;
    if (int rc = grow(p->buf[B_REFINE], refine_bytes(p) * n_cells)) return rc;
    double* q = static_cast<double*>(p->buf[B_REFINE].p);
    HIP_TRY(hommx::launch_fused2d_refine(fact, d_coef, d_M, d_corr, q, q + 8 * nn * n_cells, p->desc.n_micro, n_cells, st));
    return HOMMX_OK;
  }
  const int rc = p->family == FAM_MESH ? hommx::mesh_solve(p->mesh, n_cells, d_coef, d_M, d_A_eff, d_info, st, d_corr)
                                       : hommx::blocked_solve(p->ws, n_cells, d_coef, d_M, d_A_eff, d_info, st, d_corr);
  return rc ? route_fail(p, rc) : HOMMX_OK;
}

// a fused 2D plan forms its correctors from its own factors (route_solve); with HOMMX_FUSED_CORR=0 the first call that needs them gives it
// a workspace of the blocked family instead
int corrector_workspace(hommx_plan* p) {
  if (p->family != FAM_FUSED2D || p->ws || p->fused_corr) return HOMMX_OK;
  int rc = hommx::blocked_workspace_create(&p->ws, p->desc.dim, p->desc.n_micro, p->desc.kind);
  return rc ? prefix_error(rc, "blocked path: ") : HOMMX_OK;
}

// periodic unknowns of a cell (nodes x bs): the length of one corrector
long long plan_ndof(const hommx_plan* p) {
  const long long n = p->desc.n_micro;
  const long long nodes = p->family == FAM_MESH ? hommx::mesh_num_nodes(p->mesh) : n ? (p->desc.dim == 2 ? n * n : n * n * n) : p->ws->G.nn;
  return nodes * p->ks.bs;
}

int64_t recon_chunk(const hommx_plan* p, int64_t n_cells, size_t extra);  // below, with the reconstruction

// -- coefficient sources: inside this file a coefficient is a normalised hommx_coef_source (the pointers of its form alone) ----------------
hommx_coef_source sampled_source(const double* coef) {
  hommx_coef_source s{};
  s.form = HOMMX_COEF_SAMPLED;
  s.coef = coef;
  return s;
}
hommx_coef_source two_phase_source(const uint8_t* mask, const double* values) {
  hommx_coef_source s{};
  s.form = HOMMX_COEF_TWO_PHASE;
  s.mask = mask;
  s.values = values;
  return s;
}
hommx_coef_source separable_source(int32_t family, int32_t n_q, const double* table, const double* weights, const double* params) {
  hommx_coef_source s{};
  s.form = HOMMX_COEF_SEPARABLE;
  s.family = family;
  s.n_q = family == HOMMX_SAMPLER_AFFINE ? 1 : n_q;
  s.table = table;
  s.weights = family == HOMMX_SAMPLER_AFFINE ? nullptr : weights;
  s.params = params;
  return s;
}
hommx_coef_source program_source(const hommx_coef_program* program, int32_t n_q, const double* points, const double* weights,
                                 const double* rows, int32_t n_fields) {
  hommx_coef_source s{};
  s.form = HOMMX_COEF_PROGRAM;
  s.n_q = n_q;
  s.n_fields = n_fields;
  s.table = points;
  s.weights = weights;
  s.params = rows;
  s.program = program;
  return s;
}
// a caller's source that coef_check has passed (the pointers of other forms are not the caller's to set; `program`, the member a
// caller built against the shorter struct does not have, and `n_fields`, which was `reserved`, are read for their own form only)
hommx_coef_source source_of_form(const hommx_coef_source& s) {
  if (s.form == HOMMX_COEF_SAMPLED) return sampled_source(s.coef);
  if (s.form == HOMMX_COEF_TWO_PHASE) return two_phase_source(s.mask, s.values);
  if (s.form == HOMMX_COEF_PROGRAM) return program_source(s.program, s.n_q, s.table, s.weights, s.params, s.n_fields);
  return separable_source(s.family, s.n_q, s.table, s.weights, s.params);
}

// The whole program of a HOMMX_COEF_PROGRAM source against the plan's descriptor, on the host: the kernel then interprets it unchecked.
// load_comp: 0 for the coefficient; the tensor size t of the plan for the program of a load (HOMMX_LOADS_PROGRAM), which has t
// components on every kind.  state: 0, or the 2 t + n_comp state entries behind the fields in the row of a criterion
// (hommx_criterion_args.program): one component on every kind, and of `s` only program and n_fields are read.  state_comp: the
// components of a program on that row -- 1 for a criterion, the plan's n_comp for a law (hommx_secant_args.program), n_comp +
// n_history for a law with history variables, whose row (`state`) is longer by n_history as well (hommx_history_args)
int program_check(const hommx_plan* p, const hommx_coef_source* s, int load_comp = 0, int state = 0, int state_comp = 1) {
  if (!load_comp && !state && p->desc.kind == HOMMX_KIND_ELASTICITY_VOIGT)
    return fail(HOMMX_EINVAL, "expression coefficients are not supported for the 21-component Voigt kind");
  const hommx_coef_program* g = s->program;
  if (!g) return fail(HOMMX_EINVAL, "null program");
  if (g->n_ops < 1 || g->n_ops > hommx::PROGRAM_MAX_OPS)
    return fail(HOMMX_EINVAL, "program: n_ops must be 1 .. %d, got %d", hommx::PROGRAM_MAX_OPS, g->n_ops);
  if (g->n_consts < 0 || g->n_consts > hommx::PROGRAM_MAX_CONSTS)
    return fail(HOMMX_EINVAL, "program: n_consts must be 0 .. %d, got %d", hommx::PROGRAM_MAX_CONSTS, g->n_consts);
  if (g->n_params < 0 || g->n_params > hommx::PROGRAM_MAX_PARAMS)
    return fail(HOMMX_EINVAL, "program: n_params must be 0 .. %d, got %d", hommx::PROGRAM_MAX_PARAMS, g->n_params);
  if (g->n_params > g->n_consts)
    return fail(HOMMX_EINVAL, "program: n_params is %d, above n_consts (%d): the parameters are the first constants", g->n_params, g->n_consts);
  if (s->n_fields < 0 || s->n_fields > hommx::PROGRAM_MAX_FIELDS)
    return fail(HOMMX_EINVAL, "program source: n_fields must be 0 .. %d, got %d", hommx::PROGRAM_MAX_FIELDS, s->n_fields);
  const int n_row = hommx::program_row_doubles(s->n_fields) + state;
  const int n_comp = state ? state_comp : load_comp ? load_comp : hommx::kind_sizes(p->desc.dim, p->desc.kind).n_comp;
  if (g->n_comp != n_comp && state && state_comp == 1) return fail(HOMMX_EINVAL, "program: n_comp is %d, a criterion has one component", g->n_comp);
  if (g->n_comp != n_comp && load_comp)
    return fail(HOMMX_EINVAL, "program: n_comp is %d, a load of this plan has t = %d components", g->n_comp, n_comp);
  if (g->n_comp != n_comp && state_comp > hommx::kind_sizes(p->desc.dim, p->desc.kind).n_comp)
    return fail(HOMMX_EINVAL, "program: n_comp is %d, the plan's coefficient and the history have %d components together", g->n_comp, n_comp);
  if (g->n_comp != n_comp) return fail(HOMMX_EINVAL, "program: n_comp is %d, the plan's coefficient has %d components", g->n_comp, n_comp);
  if (!g->ops || (g->n_consts > 0 && !g->consts)) return fail(HOMMX_EINVAL, "null program ops / consts");
  if (!state) {  // a criterion is interpreted on the element's state: no quadrature rule, and its rows are the call's own argument
    if (s->n_q < 1) return fail(HOMMX_EINVAL, "program source needs n_q >= 1");
    if (!s->table || !s->weights || !s->params) return fail(HOMMX_EINVAL, "null table / weights / params");
  }
  int depth = 0;
  // a law stores every entry of the coefficient, 21 on the Voigt kind, and the updates of its history variables behind them: 25
  bool stored[std::max(hommx::PROGRAM_MAX_COMP, 21 + HOMMX_SECANT_MAX_HISTORY)] = {};
  for (int pc = 0; pc < g->n_ops; ++pc) {
    const int op = g->ops[2 * pc], k = g->ops[2 * pc + 1];
    if (op >= hommx::OP_COUNT) return fail(HOMMX_EINVAL, "program: unknown opcode %d at instruction %d", op, pc);
    if (op == hommx::OP_CONST && k >= g->n_consts)
      return fail(HOMMX_EINVAL, "program: constant index %d out of range [0,%d) at instruction %d", k, g->n_consts, pc);
    if (op == hommx::OP_X && k >= n_row) {
      if (state && state_comp > hommx::kind_sizes(p->desc.dim, p->desc.kind).n_comp)
        return fail(HOMMX_EINVAL, "program: x index %d out of range [0,%d) (the midpoint, %d fields and the 2 t + n_comp + n_history = %d "
                                  "state entries) at instruction %d", k, n_row, s->n_fields, state, pc);
      if (state)
        return fail(HOMMX_EINVAL, "program: x index %d out of range [0,%d) (the midpoint, %d fields and the 2 t + n_comp = %d state entries) "
                                  "at instruction %d", k, n_row, s->n_fields, state, pc);
      if (s->n_fields == 0) return fail(HOMMX_EINVAL, "program: x index %d out of range [0,3) at instruction %d", k, pc);
      return fail(HOMMX_EINVAL, "program: x index %d out of range [0,%d) (the midpoint and %d fields) at instruction %d", k, n_row, s->n_fields, pc);
    }
    if (op == hommx::OP_Y && k >= p->desc.dim)
      return fail(HOMMX_EINVAL, "program: y index %d out of range [0,%d) at instruction %d", k, p->desc.dim, pc);
    if (depth < hommx::op_pops(op)) return fail(HOMMX_EINVAL, "program: stack underflow at instruction %d", pc);
    depth += hommx::op_pushes(op) - hommx::op_pops(op);
    if (depth > hommx::PROGRAM_MAX_STACK)
      return fail(HOMMX_EINVAL, "program: stack depth above %d at instruction %d", hommx::PROGRAM_MAX_STACK, pc);
    if (op == hommx::OP_STORE) {
      if (k >= n_comp) return fail(HOMMX_EINVAL, "program: component index %d out of range [0,%d) at instruction %d", k, n_comp, pc);
      if (stored[k]) return fail(HOMMX_EINVAL, "program: component %d stored twice (instruction %d)", k, pc);
      stored[k] = true;
    }
  }
  if (depth != 0) return fail(HOMMX_EINVAL, "program: %d values left on the stack at the end", depth);
  for (int c = 0; c < n_comp; ++c)
    if (!stored[c]) return fail(HOMMX_EINVAL, "program: component %d never stored", c);
  return HOMMX_OK;
}

// What every entry point checks of a coefficient source: the form, its pointers, the restrictions of a separable sampler.  `separable_ptrs`
// names the pointers of the separable form as the entry point does, `more_ptrs`: the pointers it checks and names with them
int coef_check(const hommx_plan* p, const hommx_coef_source* s, const char* separable_ptrs = "table / params", bool more_ptrs = true) {
  if (!s) return fail(HOMMX_EINVAL, "null source");
  switch (s->form) {
    case HOMMX_COEF_SAMPLED: return s->coef ? HOMMX_OK : fail(HOMMX_EINVAL, "null coef");
    case HOMMX_COEF_TWO_PHASE: return s->mask && s->values ? HOMMX_OK : fail(HOMMX_EINVAL, "null mask / values");
    case HOMMX_COEF_SEPARABLE: break;
    case HOMMX_COEF_PROGRAM: return program_check(p, s);
    default: return fail(HOMMX_EINVAL, "unknown coefficient form %d", s->form);
  }
  if (p->desc.kind != HOMMX_KIND_POISSON_SCALAR && p->desc.kind != HOMMX_KIND_ELASTICITY_ISO)
    return fail(HOMMX_EINVAL, "separable samplers are defined for the scalar Poisson and the isotropic elasticity kinds");
  if (p->desc.kind == HOMMX_KIND_ELASTICITY_ISO && s->family != HOMMX_SAMPLER_AFFINE)
    return fail(HOMMX_EINVAL, "the isotropic elasticity kind takes the affine sampler only ((lambda, mu) = a + b g)");
  if (s->family != HOMMX_SAMPLER_AFFINE && s->family != HOMMX_SAMPLER_RECIPROCAL)
    return fail(HOMMX_EINVAL, "unknown sampler family %d", s->family);
  if (!s->table || !s->params || !more_ptrs) return fail(HOMMX_EINVAL, "null %s", separable_ptrs);
  if (s->family == HOMMX_SAMPLER_RECIPROCAL && (s->n_q < 1 || !s->weights))
    return fail(HOMMX_EINVAL, "reciprocal sampler needs n_q >= 1 and weights");
  return HOMMX_OK;
}

// the kernels.h form of a source, and what its kernels read per cell: the stream, or the two values / (a, b) per component
hommx::CoefSource sampler_source(const hommx_coef_source& s) {
  hommx::CoefSource src;
  if (s.form == HOMMX_COEF_TWO_PHASE) {
    src.mode = hommx::COEF_TWO_PHASE;
    src.table = s.mask;
  } else if (s.form == HOMMX_COEF_SEPARABLE) {
    src.mode = s.family == HOMMX_SAMPLER_AFFINE ? hommx::COEF_AFFINE : hommx::COEF_RECIPROCAL;
    src.nq = s.n_q;
    src.table = s.table;
    src.weights = s.weights;
  }
  return src;
}
const double* per_cell(const hommx_coef_source& s) {
  return s.form == HOMMX_COEF_SAMPLED ? s.coef : s.form == HOMMX_COEF_TWO_PHASE ? s.values : s.params;
}

// the program of a checked HOMMX_COEF_PROGRAM source as the kernel takes it
hommx::ProgramArgs program_args(const hommx_coef_program& g) {
  hommx::ProgramArgs a{};
  memcpy(a.code, g.ops, 2 * (size_t)g.n_ops);
  if (g.n_consts) memcpy(a.consts, g.consts, sizeof(double) * g.n_consts);
  a.n_ops = g.n_ops;
  a.n_comp = g.n_comp;
  return a;
}

// doubles per cell of the per-cell array of a sampler form (per_cell), and entries of its table.  A program's row is the midpoint and
// the fields of the cell (coef_program.h, program_row_doubles: nothing else knows its width); program_rows: the rows from cell c0 on
int64_t per_cell_doubles(const hommx_plan* p, const hommx_coef_source& s) {
  return s.form == HOMMX_COEF_PROGRAM ? hommx::program_row_doubles(s.n_fields) : 2 * p->ks.n_comp;
}
const double* program_rows(const hommx_coef_source& s, int64_t c0) { return s.params + c0 * hommx::program_row_doubles(s.n_fields); }
// the differentiable slots of a checked program source: its parameters, then its fields
int source_tangents(const hommx_coef_source& s) { return s.program->n_params + s.n_fields; }
// ... and the pairs a <= b of n_tan of them: the second-order streams
int tangent_pairs(int n_tan) { return n_tan * (n_tan + 1) / 2; }
// the maximal stack depth of a checked program (program_check has simulated it): the rows of the second-order kernel's stack
int program_depth(const hommx_coef_program& g) {
  int depth = 0, deepest = 0;
  for (int pc = 0; pc < g.n_ops; ++pc) {
    depth += hommx::op_pushes(g.ops[2 * pc]) - hommx::op_pops(g.ops[2 * pc]);
    deepest = std::max(deepest, depth);
  }
  return deepest;
}
int64_t table_doubles(const hommx_plan* p, const hommx_coef_source& s) {
  return p->n_el * s.n_q * (s.form == HOMMX_COEF_PROGRAM ? p->desc.dim : 1);
}

// -- the element stream of a source ---------------------------------------------------------------------------------------------------
// Cells per chunk of a source, given the `want` of the caller: a sampler form is expanded into the plan's element stream, at most 1 GiB of
// it (at least one cell), which is grown here; a sampled stream has no such limit.  n_tan: the parameter tangents of a program are
// expanded beside it (B_TANGENT), and the 1 GiB counts the 1 + n_tan streams; n_curv: its second-order streams as well (B_CURVATURE,
// with the t x t first derivatives along them behind), and the 1 GiB counts the 1 + n_tan + n_curv streams; more: doubles per cell of
// what else the device expands for the chunk (the load of HOMMX_LOADS_PROGRAM), counted with them
int64_t stream_cells(const hommx_plan* p, int64_t want, int n_tan = 0, int n_curv = 0, int64_t more = 0) {
  return std::min(want, std::max<int64_t>((1ll << 27) / std::max<int64_t>(p->n_el * p->ks.n_comp * (1 + n_tan + n_curv) + more, 1), 1));
}
int stream_chunk(hommx_plan* p, const hommx_coef_source& s, int64_t want, int64_t* chunk, int n_tan = 0, int n_curv = 0, int64_t more = 0) {
  *chunk = want;
  if (s.form == HOMMX_COEF_SAMPLED) return HOMMX_OK;
  *chunk = stream_cells(p, want, n_tan, n_curv, more);
  const size_t stream = sizeof(double) * *chunk * p->n_el * p->ks.n_comp;
  if (int rc = grow(p->buf[B_TANGENT], stream * n_tan)) return rc;
  if (int rc = grow(p->buf[B_CURVATURE], (stream + sizeof(double) * *chunk * p->ks.t * p->ks.t) * n_curv)) return rc;
  return grow(p->buf[B_EXPAND], stream);
}

// *stream: the element stream of cells [c0, c0 + nc) of a source on the device.  A sampled stream is a view of the caller's; a sampler
// form is expanded into the plan's element stream (nc <= the chunk of stream_chunk) or, if given, into `into`; `tangents`: a program's
// parameter tangents as well, in the same launch -- and then a null `stream`: the tangents alone, no element stream is written;
// `curvature`: the second-order pass instead, which writes the second-order streams and, where given, the stream and the tangents
int expand_chunk(hommx_plan* p, const hommx_coef_source& s, int64_t c0, int64_t nc, hipStream_t st, const double** stream,
                 double* into = nullptr, double* tangents = nullptr, double* curvature = nullptr) {
  const int n_comp = p->ks.n_comp;
  if (s.form == HOMMX_COEF_SAMPLED) {
    *stream = s.coef + c0 * p->n_el * n_comp;
    return HOMMX_OK;
  }
  double* dst = !stream ? nullptr : into ? into : static_cast<double*>(p->buf[B_EXPAND].p);
  if (s.form == HOMMX_COEF_TWO_PHASE)
    HIP_TRY(hommx::launch_expand_two_phase(s.mask, s.values + c0 * 2 * n_comp, dst, p->n_el, n_comp, nc, st));
  else if (s.form == HOMMX_COEF_PROGRAM && curvature)
    HIP_TRY(hommx::launch_expand_program2(program_args(*s.program), s.program->n_params, s.n_fields, program_depth(*s.program), s.table,
                                          s.weights, s.n_q, p->desc.dim, program_rows(s, c0), dst, tangents, curvature, p->n_el, nc, st));
  else if (s.form == HOMMX_COEF_PROGRAM)
    HIP_TRY(hommx::launch_expand_program(program_args(*s.program), s.program->n_params, s.n_fields, s.table, s.weights, s.n_q, p->desc.dim,
                                         program_rows(s, c0), dst, tangents, p->n_el, nc, st));
  else
    HIP_TRY(hommx::launch_expand_separable(sampler_source(s), s.params + c0 * 2 * n_comp, dst, p->n_el, n_comp, nc, st));
  if (stream) *stream = dst;
  return HOMMX_OK;
}

// A source on the device, solved: what the *_device solve entry points do.  The fused 2D kernel samples the two-phase and separable
// forms itself; a program is expanded chunk by chunk and solved in the kernel's STREAM mode.  The other families read an element
// stream: a sampled one goes to the route in one call, a sampler form chunk by chunk of stream_chunk
int solve_source_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source& s, const double* d_M, double* d_A_eff, int32_t* d_info,
                        hipStream_t st) {
  const bool fused = p->family == FAM_FUSED2D;
  if (fused && s.form != HOMMX_COEF_PROGRAM) {
    HIP_TRY(hommx::launch_poisson2d_fused(per_cell(s), d_M, d_A_eff, d_info, p->desc.n_micro, n_cells, st, sampler_source(s)));
    return HOMMX_OK;
  }
  int64_t chunk = 0;
  if (int rc = stream_chunk(p, s, n_cells, &chunk)) return rc;
  const int d = p->desc.dim, t = p->ks.t;
  for (int64_t c0 = 0; c0 < n_cells; c0 += chunk) {
    const int64_t nc = (n_cells - c0 < chunk) ? n_cells - c0 : chunk;
    const double* stream = nullptr;
    if (int rc = expand_chunk(p, s, c0, nc, st, &stream)) return rc;
    const double* M = d_M ? d_M + c0 * d * d : nullptr;
    int32_t* info = d_info ? d_info + c0 : nullptr;
    if (fused) {
      HIP_TRY(hommx::launch_poisson2d_fused(stream, M, d_A_eff + c0 * t * t, info, p->desc.n_micro, nc, st));
      continue;
    }
    if (int rc = route_solve(p, nc, stream, M, d_A_eff + c0 * t * t, info, st)) return rc;
  }
  return HOMMX_OK;
}

// -- the sampler host entry points ------------------------------------------------------------------------------------------------------
// Their inputs are small, so they are packed into ONE pinned block owned by the plan and travel in one asynchronous copy to its device
// twin: no hipMalloc / hipFree per call.  A null input takes no room; *dst of a piece: its device copy (null for a null input)
template <size_t N>
int stage_in(hommx_plan* p, const hommx::HostPiece (&in)[N]) {
  size_t bytes[N], total = 0;
  char *pin[N], *dev[N];
  for (size_t k = 0; k < N; ++k) bytes[k] = in[k].src ? in[k].bytes : 0;
  if (int rc = carve(p->buf[B_PIN_IN], bytes, pin, &total)) return rc;
  if (int rc = carve(p->buf[B_DEV_IN], bytes, dev)) return rc;
  for (size_t k = 0; k < N; ++k) {
    *in[k].dst = dev[k];
    if (bytes[k]) memcpy(pin[k], in[k].src, bytes[k]);
  }
  if (total) HIP_TRY(hipMemcpyAsync(p->buf[B_DEV_IN].p, p->buf[B_PIN_IN].p, total, hipMemcpyHostToDevice, nullptr));
  return HOMMX_OK;
}

// The host arrays of a source staged so (what every cell shares and the per-cell values of a sampler form; a sampled stream stays where
// it is, and ds->coef is null: the stream is no device pointer), with one more input of the entry point; *ds: the source with the
// device copies; load: the program source of a load (HOMMX_LOADS_PROGRAM) or null -- its points, weights and rows travel in the same
// copy and their device copies replace its pointers
int stage_source(hommx_plan* p, int64_t n_cells, const hommx_coef_source& s, hommx::HostPiece more, hommx_coef_source* ds,
                 hommx_coef_source* load = nullptr) {
  const size_t nval = sizeof(double) * n_cells * per_cell_doubles(p, s);
  *ds = s;
  ds->coef = nullptr;
  hommx_coef_source none{};
  const hommx_coef_source host = load ? *load : none;
  hommx_coef_source& dl = load ? *load : none;  // without a load its three pieces are empty
  const hommx::HostPiece in[] = {{s.mask, (size_t)p->n_el, (const void**)&ds->mask},
                                 {s.values, nval, (const void**)&ds->values},
                                 {s.table, sizeof(double) * table_doubles(p, s), (const void**)&ds->table},
                                 {s.weights, sizeof(double) * s.n_q, (const void**)&ds->weights},
                                 {s.params, nval, (const void**)&ds->params},
                                 more,
                                 {host.table, load ? sizeof(double) * table_doubles(p, host) : 0, (const void**)&dl.table},
                                 {host.weights, sizeof(double) * host.n_q, (const void**)&dl.weights},
                                 {host.params, load ? sizeof(double) * n_cells * per_cell_doubles(p, host) : 0, (const void**)&dl.params}};
  return stage_in(p, in);
}

// hommx_solve_batch_two_phase / _separable / _source: the source and M go in staged, the outputs come back the same way, the call synchronises once
int solve_source_host(hommx_plan* p, int64_t n_cells, const hommx_coef_source& s, const double* M, double* A_eff, int32_t* info) {
  const int d = p->desc.dim;
  const size_t out_bytes[] = {sizeof(double) * n_cells * p->ks.t * p->ks.t, sizeof(int32_t) * n_cells};
  size_t total = 0;
  char *pin[2], *dev[2];
  if (int rc = carve(p->buf[B_PIN_OUT], out_bytes, pin, &total)) return rc;
  if (int rc = carve(p->buf[B_DEV_OUT], out_bytes, dev)) return rc;
  hommx_coef_source ds;
  const double* d_M = nullptr;
  if (int rc = stage_source(p, n_cells, s, {M, sizeof(double) * n_cells * d * d, (const void**)&d_M}, &ds)) return rc;
  if (int rc = one_launch_check(n_cells)) return rc;  // what the device entry point this call stands for would say here
  if (int rc = solve_source_device(p, n_cells, ds, d_M, reinterpret_cast<double*>(dev[0]), reinterpret_cast<int32_t*>(dev[1]), nullptr)) return rc;
  HIP_TRY(hipMemcpyAsync(pin[0], dev[0], total, hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  memcpy(A_eff, pin[0], out_bytes[0]);
  if (info) memcpy(info, pin[1], out_bytes[1]);
  return HOMMX_OK;
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
  const int dim = d->dim, n = d->n_micro;
  hommx_plan* p = nullptr;
  if (int rc = plan_new(&p, *d, (dim == 2) ? 2ll * n * n : 6ll * n * n * n)) return rc;
  const bool fused = dim == 2 && d->kind == HOMMX_KIND_POISSON_SCALAR && n <= 32 && !(d->flags & HOMMX_FLAG_FORCE_BLOCKED);
  p->family = fused ? FAM_FUSED2D : FAM_BLOCKED;
  if (p->family == FAM_BLOCKED) {
    int rc = hommx::blocked_workspace_create(&p->ws, dim, n, d->kind);
    if (rc != 0) {
      delete p;
      return prefix_error(rc, "blocked path: ");
    }
    if (d->flags & HOMMX_FLAG_TREE_LOADS) hommx::blocked_enable_tree_loads(p->ws);
  }
  *out = p;
  return HOMMX_OK;
}

int hommx_plan_destroy(hommx_plan* p) {
  if (!p) return HOMMX_OK;
  hipSetDevice(p->desc.device);
  if (p->ws) hommx::blocked_workspace_destroy(p->ws);
  if (p->mesh) hommx::mesh_destroy(p->mesh);
  for (Buf& b : p->buf) b.release();
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

const char* hommx_plan_corrector_kernel_name(const hommx_plan* p) {
  if (!p) return "";
  switch (p->family) {
    case FAM_FUSED2D: return p->fused_corr ? "fused2d_subst" : "blocked";
    case FAM_MESH: return "mesh_front";
    default: return hommx::blocked_corrector_route_name(p->ws);
  }
}

const char* hommx_plan_load_kernel_name(const hommx_plan* p) {
  if (!p) return "";
  switch (p->family) {
    case FAM_FUSED2D: return fused_loads(p) ? "fused2d_subst" : "blocked";
    case FAM_MESH: return mesh_loads(p) ? "mesh_front_subst" : "none";
    default: return hommx::blocked_load_route_name(p->ws);  // "multifrontal_subst" / "mesh_multifrontal_subst" with the flag on a tree plan
  }
}

const char* hommx_plan_route_detail(hommx_plan* p) {
  if (!p) return "";
  switch (p->family) {
    case FAM_FUSED2D:
      return p->desc.n_micro > 16 ? "fused2d: k_poisson2d_fused<32, false>, one wavefront per macro cell, every matrix in the f64 MFMA accumulator layout"
                                  : "fused2d: k_poisson2d_fused<16, false>, one wavefront per macro cell, every matrix in the f64 MFMA accumulator layout";
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
  hommx_plan_desc desc{};  // n_micro == 0: a mesh plan
  desc.dim = d->dim;
  desc.kind = d->kind;
  desc.device = d->device;
  desc.flags = m ? d->flags : d->flags | HOMMX_MESH_FLAG_TREE;  // the descriptor names the route the plan took
  hommx_plan* p = nullptr;
  if ((rc = plan_new(&p, desc, d->n_el)) != 0) {
    hommx::mesh_destroy(m);
    hommx::mesh_tree_destroy(mt);
    return rc;
  }
  p->family = m ? FAM_MESH : FAM_BLOCKED;
  p->mesh = m;
  rc = hipSetDevice(d->device) == hipSuccess ? HOMMX_OK : fail(HOMMX_EHIP, "hipSetDevice failed");
  if (!rc) rc = hommx::mesh_geom_upload(d, geo, &p->geo);
  if (!rc) rc = m ? hommx::mesh_upload(m, p->geo) : hommx::mesh_tree_workspace(mt, p->geo, &p->ws);
  hommx::mesh_tree_destroy(mt);  // host analysis only: the workspace holds what the tree route needs
  if (!rc && !m && (d->flags & HOMMX_MESH_FLAG_TREE_LOADS)) hommx::blocked_enable_tree_loads(p->ws);
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
  return solve_source_device(p, n_cells, sampled_source(d_coef), d_M, d_A_eff, d_info, reinterpret_cast<hipStream_t>(stream));
}

int hommx_solve_batch(hommx_plan* p, int64_t n_cells, const double* coef, const double* M, double* A_eff,
                      int32_t* info) {
  if (int rc = open_call(p, n_cells, coef && A_eff, "coef / A_eff"); rc != GO) return rc;
  const int d = p->desc.dim, t = p->ks.t;
  const int64_t per = p->n_el * p->ks.n_comp;
  const size_t in_bytes[] = {sizeof(double) * n_cells * per, M ? sizeof(double) * n_cells * d * d : 0};
  const size_t out_bytes[] = {sizeof(double) * n_cells * t * t, sizeof(int32_t) * n_cells};
  char *in[2], *out[2];
  if (int rc = carve(p->buf[B_IN], in_bytes, in)) return rc;
  if (int rc = carve(p->buf[B_OUT], out_bytes, out)) return rc;
  double* d_coef = reinterpret_cast<double*>(in[0]);
  double* d_M = reinterpret_cast<double*>(in[1]);
  double* d_out = reinterpret_cast<double*>(out[0]);
  int32_t* d_info = reinterpret_cast<int32_t*>(out[1]);
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
  return solve_source_device(p, n_cells, two_phase_source(d_mask, d_values), d_M, d_A_eff, d_info, reinterpret_cast<hipStream_t>(stream));
}

int hommx_solve_batch_two_phase(hommx_plan* p, int64_t n_cells, const uint8_t* mask, const double* values,
                                const double* M, double* A_eff, int32_t* info) {
  if (int rc = open_call(p, n_cells, mask && values && A_eff, "mask / values / A_eff"); rc != GO) return rc;
  return solve_source_host(p, n_cells, two_phase_source(mask, values), M, A_eff, info);
}

int hommx_solve_batch_separable_device(hommx_plan* p, int64_t n_cells, int32_t family, int32_t n_q, const double* d_table,
                                       const double* d_weights, const double* d_params, const double* d_M, double* d_A_eff,
                                       int32_t* d_info, void* stream) {
  const char* names = "table / params / A_eff";  // kind, family, pointers, n_q and weights: the order this entry always had
  const hommx_coef_source s = separable_source(family, n_q, d_table, d_weights, d_params);
  if (int rc = open_call(p, n_cells, true, "", true, [&] { return coef_check(p, &s, names, d_A_eff); }); rc != GO) return rc;
  return solve_source_device(p, n_cells, s, d_M, d_A_eff, d_info, reinterpret_cast<hipStream_t>(stream));
}

int hommx_solve_batch_separable(hommx_plan* p, int64_t n_cells, int32_t family, int32_t n_q, const double* table,
                                const double* weights, const double* params, const double* M, double* A_eff, int32_t* info) {
  const char* names = "table / params / A_eff";
  const hommx_coef_source s = separable_source(family, n_q, table, weights, params);
  if (int rc = open_call(p, n_cells, true, "", false, [&] { return coef_check(p, &s, names, A_eff); }); rc != GO) return rc;
  return solve_source_host(p, n_cells, s, M, A_eff, info);
}

int hommx_solve_batch_source_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* d_M, double* d_A_eff,
                                    int32_t* d_info, void* stream) {
  if (int rc = open_call(p, n_cells, d_A_eff, "A_eff", true, [&] { return coef_check(p, src); }); rc != GO) return rc;
  return solve_source_device(p, n_cells, source_of_form(*src), d_M, d_A_eff, d_info, reinterpret_cast<hipStream_t>(stream));
}

int hommx_solve_batch_source(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* M, double* A_eff, int32_t* info) {
  if (int rc = open_call(p, n_cells, A_eff, "A_eff", false, [&] { return coef_check(p, src); }); rc != GO) return rc;
  if (src->form == HOMMX_COEF_SAMPLED) return hommx_solve_batch(p, n_cells, src->coef, M, A_eff, info);  // the pipelined copy of the stream
  return solve_source_host(p, n_cells, source_of_form(*src), M, A_eff, info);
}

int hommx_expand_source_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, double* d_coef_out, void* stream) {
  if (int rc = open_call(p, n_cells, d_coef_out, "coef_out", true, [&] { return coef_check(p, src); }); rc != GO) return rc;
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const hommx_coef_source s = source_of_form(*src);
  const int64_t per = p->n_el * p->ks.n_comp;
  if (s.form == HOMMX_COEF_SAMPLED) {
    HIP_TRY(hipMemcpyAsync(d_coef_out, s.coef, sizeof(double) * n_cells * per, hipMemcpyDeviceToDevice, st));
    return HOMMX_OK;
  }
  const int64_t chunk = stream_cells(p, n_cells);  // straight into the caller's array, in launches of at most 1 GiB of stream
  for (int64_t c0 = 0; c0 < n_cells; c0 += chunk) {
    const double* at = nullptr;
    if (int rc = expand_chunk(p, s, c0, std::min(chunk, n_cells - c0), st, &at, d_coef_out + c0 * per)) return rc;
  }
  return HOMMX_OK;
}

int hommx_expand_source(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, double* coef_out) {
  if (int rc = open_call(p, n_cells, coef_out, "coef_out", false, [&] { return coef_check(p, src); }); rc != GO) return rc;
  const hommx_coef_source s = source_of_form(*src);
  const int64_t per = p->n_el * p->ks.n_comp;
  if (s.form == HOMMX_COEF_SAMPLED) {
    memcpy(coef_out, s.coef, sizeof(double) * n_cells * per);
    return HOMMX_OK;
  }
  hommx_coef_source ds;
  const void* none = nullptr;
  if (int rc = stage_source(p, n_cells, s, {nullptr, 0, &none}, &ds)) return rc;
  int64_t chunk = 0;
  if (int rc = stream_chunk(p, s, n_cells, &chunk)) return rc;
  for (int64_t c0 = 0; c0 < n_cells; c0 += chunk) {
    const int64_t nc = std::min(chunk, n_cells - c0);
    const double* at = nullptr;
    if (int rc = expand_chunk(p, ds, c0, nc, nullptr, &at)) return rc;
    HIP_TRY(hipMemcpyAsync(coef_out + c0 * per, at, sizeof(double) * nc * per, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
  }
  return HOMMX_OK;
}

}  // extern "C"

namespace {
// the differentiable slots of a checked program source, 1 .. HOMMX_PROGRAM_MAX_PARAMS of them: its parameters, then its fields
int tangent_slots_check(const hommx_coef_source* s, const char* who) {
  const int n_params = s->program->n_params, n_fields = s->n_fields;
  if (n_params + n_fields == 0) return fail(HOMMX_EINVAL, "%s: the program has no parameters (n_params == 0)", who);
  if (n_params + n_fields > HOMMX_PROGRAM_MAX_PARAMS)
    return fail(HOMMX_EINVAL, "%s: at most %d differentiable slots, got n_params (%d) + n_fields (%d) = %d", who, HOMMX_PROGRAM_MAX_PARAMS,
                n_params, n_fields, n_params + n_fields);
  return HOMMX_OK;
}
// what hommx_expand_tangents[_device] check of the source beyond coef_check
int tangents_check(const hommx_plan* p, const hommx_coef_source* src) {
  if (int rc = coef_check(p, src)) return rc;
  if (src->form != HOMMX_COEF_PROGRAM) return fail(HOMMX_EINVAL, "parameter tangents need a HOMMX_COEF_PROGRAM source, got form %d", src->form);
  return tangent_slots_check(src, "parameter tangents");
}
}  // namespace

extern "C" {

int hommx_expand_tangents_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, double* d_coef_out, double* d_dirs_out,
                                 void* stream) {
  if (int rc = open_call(p, n_cells, d_dirs_out, "dirs_out", true, [&] { return tangents_check(p, src); }); rc != GO) return rc;
  const hommx_coef_source s = source_of_form(*src);
  const int n_tan = source_tangents(s);
  const int64_t per = p->n_el * p->ks.n_comp;
  const int64_t chunk = stream_cells(p, n_cells, n_tan);  // straight into the caller's arrays, in launches of at most 1 GiB of streams
  for (int64_t c0 = 0; c0 < n_cells; c0 += chunk) {
    const double* at = nullptr;
    if (int rc = expand_chunk(p, s, c0, std::min(chunk, n_cells - c0), reinterpret_cast<hipStream_t>(stream), d_coef_out ? &at : nullptr,
                              d_coef_out ? d_coef_out + c0 * per : nullptr, d_dirs_out + c0 * n_tan * per))
      return rc;
  }
  return HOMMX_OK;
}

int hommx_expand_tangents(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, double* coef_out, double* dirs_out) {
  if (int rc = open_call(p, n_cells, dirs_out, "dirs_out", false, [&] { return tangents_check(p, src); }); rc != GO) return rc;
  const hommx_coef_source s = source_of_form(*src);
  const int n_tan = source_tangents(s);
  const int64_t per = p->n_el * p->ks.n_comp;
  hommx_coef_source ds;
  const void* none = nullptr;
  if (int rc = stage_source(p, n_cells, s, {nullptr, 0, &none}, &ds)) return rc;
  int64_t chunk = 0;
  if (int rc = stream_chunk(p, s, n_cells, &chunk, n_tan)) return rc;
  double* d_dirs = static_cast<double*>(p->buf[B_TANGENT].p);
  for (int64_t c0 = 0; c0 < n_cells; c0 += chunk) {
    const int64_t nc = std::min(chunk, n_cells - c0);
    const double* d_coef = nullptr;
    if (int rc = expand_chunk(p, ds, c0, nc, nullptr, coef_out ? &d_coef : nullptr, nullptr, d_dirs)) return rc;
    if (coef_out) HIP_TRY(hipMemcpyAsync(coef_out + c0 * per, d_coef, sizeof(double) * nc * per, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipMemcpyAsync(dirs_out + c0 * n_tan * per, d_dirs, sizeof(double) * nc * n_tan * per, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
  }
  return HOMMX_OK;
}

int hommx_expand_second_tangents_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, double* d_coef_out, double* d_dirs_out,
                                        double* d_curv_out, void* stream) {
  if (int rc = open_call(p, n_cells, d_curv_out, "curv_out", true, [&] { return tangents_check(p, src); }); rc != GO) return rc;
  const hommx_coef_source s = source_of_form(*src);
  const int n_tan = source_tangents(s), n_pairs = tangent_pairs(n_tan);
  const int64_t per = p->n_el * p->ks.n_comp;
  const int64_t chunk = stream_cells(p, n_cells, n_tan, n_pairs);  // straight into the caller's arrays, in launches of at most 1 GiB of streams
  for (int64_t c0 = 0; c0 < n_cells; c0 += chunk) {
    const double* at = nullptr;
    if (int rc = expand_chunk(p, s, c0, std::min(chunk, n_cells - c0), reinterpret_cast<hipStream_t>(stream), d_coef_out ? &at : nullptr,
                              d_coef_out ? d_coef_out + c0 * per : nullptr, d_dirs_out ? d_dirs_out + c0 * n_tan * per : nullptr,
                              d_curv_out + c0 * n_pairs * per))
      return rc;
  }
  return HOMMX_OK;
}

int hommx_expand_second_tangents(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, double* coef_out, double* dirs_out,
                                 double* curv_out) {
  if (int rc = open_call(p, n_cells, curv_out, "curv_out", false, [&] { return tangents_check(p, src); }); rc != GO) return rc;
  const hommx_coef_source s = source_of_form(*src);
  const int n_tan = source_tangents(s), n_pairs = tangent_pairs(n_tan);
  const int64_t per = p->n_el * p->ks.n_comp;
  hommx_coef_source ds;
  const void* none = nullptr;
  if (int rc = stage_source(p, n_cells, s, {nullptr, 0, &none}, &ds)) return rc;
  int64_t chunk = 0;
  if (int rc = stream_chunk(p, s, n_cells, &chunk, n_tan, n_pairs)) return rc;
  double *d_dirs = static_cast<double*>(p->buf[B_TANGENT].p), *d_curv = static_cast<double*>(p->buf[B_CURVATURE].p);
  for (int64_t c0 = 0; c0 < n_cells; c0 += chunk) {
    const int64_t nc = std::min(chunk, n_cells - c0);
    const double* d_coef = nullptr;
    if (int rc = expand_chunk(p, ds, c0, nc, nullptr, coef_out ? &d_coef : nullptr, nullptr, dirs_out ? d_dirs : nullptr, d_curv)) return rc;
    if (coef_out) HIP_TRY(hipMemcpyAsync(coef_out + c0 * per, d_coef, sizeof(double) * nc * per, hipMemcpyDeviceToHost, nullptr));
    if (dirs_out) HIP_TRY(hipMemcpyAsync(dirs_out + c0 * n_tan * per, d_dirs, sizeof(double) * nc * n_tan * per, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipMemcpyAsync(curv_out + c0 * n_pairs * per, d_curv, sizeof(double) * nc * n_pairs * per, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
  }
  return HOMMX_OK;
}

int hommx_solve_batch_correctors(hommx_plan* p, int64_t n_cells, const double* coef, const double* M, double* A_eff,
                                 double* correctors, int32_t* info) {
  if (int rc = open_call(p, n_cells, coef && A_eff && correctors, "coef / A_eff / correctors"); rc != GO) return rc;
  if (int rc = corrector_workspace(p)) return rc;
  const int d = p->desc.dim, t = p->ks.t;
  // the call's own device block, freed when it returns: the correctors can run to gigabytes, the plan keeps none of them
  struct CallBuf : Buf {
    ~CallBuf() { release(); }
  } block;
  const size_t bytes[] = {sizeof(double) * n_cells * p->n_el * p->ks.n_comp, M ? sizeof(double) * n_cells * d * d : 0,
                          sizeof(double) * n_cells * t * t, sizeof(double) * n_cells * t * plan_ndof(p), sizeof(int32_t) * n_cells};
  char* at[5];
  if (int rc = carve(block, bytes, at)) return rc;
  HIP_TRY(hipMemcpy(at[0], coef, bytes[0], hipMemcpyHostToDevice));
  if (M) HIP_TRY(hipMemcpy(at[1], M, bytes[1], hipMemcpyHostToDevice));
  // one call into the route; a fused 2D plan on its own route: chunks whose factor records and correctors fit HOMMX_RECON_MEM_MB
  const int64_t chunk = fused_subst(p) ? recon_chunk(p, n_cells, 0) : n_cells;
  const double *d_coef = reinterpret_cast<const double*>(at[0]), *d_M = reinterpret_cast<const double*>(at[1]);
  double *d_A = reinterpret_cast<double*>(at[2]), *d_corr = reinterpret_cast<double*>(at[3]);
  int32_t* d_info = reinterpret_cast<int32_t*>(at[4]);
  for (int64_t c0 = 0; c0 < n_cells; c0 += chunk) {
    int rc = route_solve(p, std::min(chunk, n_cells - c0), d_coef + c0 * p->n_el * p->ks.n_comp, d_M ? d_M + c0 * d * d : nullptr,
                         d_A + c0 * t * t, d_info + c0, nullptr, d_corr + c0 * t * plan_ndof(p));
    if (rc != HOMMX_OK) return rc;
  }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(A_eff, at[2], bytes[2], hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(correctors, at[3], bytes[3], hipMemcpyDeviceToHost));
  if (info) HIP_TRY(hipMemcpy(info, at[4], bytes[4], hipMemcpyDeviceToHost));
  return HOMMX_OK;
}

}  // extern "C"

namespace {

bool recon_in_lds(const hommx_plan* p) { return sizeof(double) * plan_ndof(p) <= hommx::recon_lds_limit(); }

// cells per chunk: HOMMX_RECON_MEM_MB of correctors (with the chi^xi slots of cells too large for LDS), of the factor records of a fused
// 2D plan's own corrector route with its refinement scratch, and of `extra` bytes per cell
int64_t recon_chunk(const hommx_plan* p, int64_t n_cells, size_t extra) {
  const long long nd = plan_ndof(p);
  const size_t per = sizeof(double) * nd * (p->ks.t + (recon_in_lds(p) ? 0 : 1)) + fact_bytes(p) + refine_bytes(p) + extra;
  return std::clamp<int64_t>((int64_t)((p->recon_mem_mb << 20) / per), 1, n_cells);
}

// cells per chunk of an entry point whose chunks end in a load solve (load_correctors): the chunk rule of the reconstruction, and on a
// flagged frontal mesh plan the pivot columns of the arena as well, at most one arena chunk of them -- mesh_solve then runs the chunk as
// one arena chunk and its columns are still there when the load pass reads them; on a flagged plan of a tree route likewise at most one
// arena chunk of its corrector plan (reserved here for the chunk the reconstruction's rule gives, as the first solve would), whose fronts
// mf_solve then leaves whole
int64_t load_chunk(const hommx_plan* p, int64_t n_cells, size_t extra) {
  if (tree_loads(p)) {
    const int64_t chunk = recon_chunk(p, n_cells, extra), arena = hommx::blocked_tree_load_chunk(p->ws, chunk);
    return arena > 0 ? std::min(chunk, arena) : chunk;
  }
  if (!mesh_loads(p)) return recon_chunk(p, n_cells, extra);
  return std::min<int64_t>(recon_chunk(p, n_cells, extra + hommx::mesh_arena_bytes_per_cell(p->mesh)), hommx::mesh_arena_chunk(p->mesh, n_cells));
}

// The correctors of one chunk (nc of at most `chunk` cells) through the plan's route into its scratch, with room for `slots` more vectors
// of ndof per cell behind them; A_eff into *d_A_eff or, if that is null, into the plan's own array (*d_A_eff then names it)
int chunk_correctors(hommx_plan* p, int64_t nc, int64_t chunk, const double* d_coef, const double* d_M, double** d_A_eff, int32_t* d_info,
                     int slots, hipStream_t st, double** corr) {
  const int t = p->ks.t;
  if (int rc = grow(p->buf[B_RCORR], sizeof(double) * chunk * plan_ndof(p) * (t + slots))) return rc;
  if (!*d_A_eff) {
    if (int rc = grow(p->buf[B_RA], sizeof(double) * chunk * t * t)) return rc;
    *d_A_eff = static_cast<double*>(p->buf[B_RA].p);
  }
  *corr = static_cast<double*>(p->buf[B_RCORR].p);
  return route_solve(p, nc, d_coef, d_M, *d_A_eff, d_info, st, *corr);
}

// what a kernel that walks the elements reads of the plan (hommx::ElemWalk, the base of its arguments): dim, kind and the element
// geometry, which structured plans compute and mesh plans read from the plan's geometry block
void set_geometry(const hommx_plan* p, hommx::ElemWalk& a) {
  a.dim = p->desc.dim;
  a.kind = p->desc.kind;
  a.mesh = p->desc.n_micro == 0;
  a.ndof = plan_ndof(p);
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
}

// -- the derived outputs: one chunk driver under reconstruction, first derivatives, stratification, loads, second derivatives -------------
// One per-cell array of a call.  `slot` is a pointer member of the chunk's view (Chunk::a, a copy of the caller's argument struct): it
// holds the caller's pointer when the call starts (null: absent, as is an array of n == 0) and receives the chunk's device pointer.
// n: elements of `elem` bytes per cell.  SHARED (an input, at most one per call): one array of n elements serves every cell.  KEPT (an
// output): it has room in a host call's B_OUT even if the caller does not ask for it (A_eff, info).
enum ArrayKind { PER_CELL, SHARED, KEPT };
struct CellArray {
  void* slot;
  int64_t n;
  ArrayKind kind = PER_CELL;
  size_t elem = sizeof(double);
  char* get() const {
    char* q;
    memcpy(&q, slot, sizeof(q));
    return q;
  }
  void set(const void* q) const { memcpy(slot, &q, sizeof(q)); }
};

// what a family's run sees of one chunk: the element stream and M of its cells, the source on the device (for what every cell shares),
// and the caller's arguments with every pointer re-based to the chunk
template <typename Args>
struct Chunk {
  const double *coef, *M;
  const hommx_coef_source* src;
  Args a;
  double* curv = nullptr;  // HOMMX_DIRS_PARAMETERS_CURVATURE: the second-order streams of the chunk (B_CURVATURE), else null
};

using ChunkRule = int64_t (*)(const hommx_plan*, int64_t, size_t);  // recon_chunk or load_chunk

// The chunk loop of every derived output.  v.a holds the caller's arguments; `ins` / `outs` list its per-cell arrays in the order of the
// blocks of B_IN = [coef | M | ins] and B_OUT = [outs | info]; `scratch`: bytes per cell a chunk holds beside the canonical correctors.
// Per chunk of cells [c0, c0 + nc): every slot is re-based, expand_chunk gives the element stream of a sampler form, run(nc, chunk, v) forms
// the correctors and launches the family's kernels.
// device: the slots become views of the caller's arrays (pointer + c0 * n; a shared input as it is), everything on `st`, no copy and no
// synchronisation.
// host: what every cell shares (mask, table, weights of the source, the shared input) and the per-cell values of a sampler form travel
// once, in the plan's pinned block (stage_source); the other inputs stream into B_IN and the outputs the caller asked for stream out of
// B_OUT chunk by chunk, so device memory is bounded by the chunk, whose bytes per cell count both blocks.
// tangents (HOMMX_DIRS_PARAMETERS): a pointer member of v.a that receives, per chunk, the parameter tangents of the program source --
// [nc][n_params + n_fields][n_el][n_comp] in B_TANGENT, formed by the launch that expands the stream; their bytes count as scratch of the chunk
// curvature (HOMMX_DIRS_PARAMETERS_CURVATURE, with tangents): that launch is the second-order pass and also forms the second-order
// streams of the chunk, [nc][n_pairs][n_el][n_comp] in B_CURVATURE (v.curv), whose bytes count as scratch too
// load (HOMMX_LOADS_PROGRAM): a program source of the call's own beside the coefficient's, and the pointer member of v.a that receives,
// per chunk, its expansion on the rows of the chunk's cells -- [nc][n_el][n_comp of its program] in B_POLAR, the value pass of the
// interpreter; a host call stages its points, weights and rows with the coefficient source's shared arrays.  The caller counts its
// bytes in `scratch`; the 1 GiB bound of stream_chunk counts them with the streams
struct ProgramLoad {
  hommx_coef_source src;
  const double** slot;
};
template <typename Args, size_t NI, size_t NO, typename Run>
int derived_call(hommx_plan* p, int64_t n_cells, const hommx_coef_source& s, const double* M, Chunk<Args>& v, const CellArray (&ins)[NI],
                 const CellArray (&outs)[NO], int32_t** info, size_t scratch, ChunkRule rule, bool device, hipStream_t st, Run run,
                 const double** tangents = nullptr, bool curvature = false, ProgramLoad* load = nullptr) {
  const int n_tan = tangents ? source_tangents(s) : 0, n_curv = curvature ? tangent_pairs(n_tan) : 0;
  const int64_t load_doubles = load ? p->n_el * load->src.program->n_comp : 0;
  scratch += sizeof(double) * (n_tan * p->n_el * p->ks.n_comp + n_curv * (p->n_el * p->ks.n_comp + p->ks.t * p->ks.t));
  constexpr size_t N[2] = {NI + 2, NO + 1};
  constexpr size_t NMAX = std::max(N[0], N[1]);
  v.coef = s.coef;
  v.M = M;
  CellArray tab[2][NMAX] = {{{&v.coef, s.form == HOMMX_COEF_SAMPLED ? p->n_el * p->ks.n_comp : 0}, {&v.M, p->desc.dim * p->desc.dim}}, {}};
  std::copy(ins, ins + NI, tab[0] + 2);
  std::copy(outs, outs + NO, tab[1]);
  tab[1][NO] = CellArray{info, 1, KEPT, sizeof(int32_t)};
  // the caller's pointers, and the bytes per cell of those that take room in a chunk
  char* user[2][NMAX];
  size_t cell[2][NMAX], per_cell = scratch;
  const CellArray* shared = nullptr;
  for (int io = 0; io < 2; ++io)
    for (size_t k = 0; k < N[io]; ++k) {
      const CellArray& c = tab[io][k];
      user[io][k] = c.get();
      if (c.kind == SHARED) shared = &c;
      cell[io][k] = c.kind != SHARED && (user[io][k] || c.kind == KEPT) ? c.elem * c.n : 0;
      per_cell += cell[io][k];
    }
  hommx_coef_source ds = s;
  char* dev[2][NMAX] = {};
  int64_t chunk = 0;
  if (device) {
    if (int rc = stream_chunk(p, s, rule(p, n_cells, scratch), &chunk, n_tan, n_curv, load_doubles)) return rc;
  } else {
    const void* d_shared = nullptr;
    const hommx::HostPiece more{shared ? shared->get() : nullptr, shared ? shared->elem * shared->n : 0, &d_shared};
    if (int rc = stage_source(p, n_cells, s, more, &ds, load ? &load->src : nullptr)) return rc;
    if (shared) shared->set(d_shared);
    if (int rc = stream_chunk(p, s, rule(p, n_cells, per_cell), &chunk, n_tan, n_curv, load_doubles)) return rc;
    for (int io = 0; io < 2; ++io) {
      size_t bytes[NMAX] = {};
      for (size_t k = 0; k < N[io]; ++k) bytes[k] = cell[io][k] * chunk;
      if (int rc = carve(p->buf[io ? B_OUT : B_IN], bytes, dev[io])) return rc;
    }
  }
  v.src = &ds;
  if (load)
    if (int rc = grow(p->buf[B_POLAR], sizeof(double) * chunk * load_doubles)) return rc;
  for (int64_t c0 = 0; c0 < n_cells; c0 += chunk) {
    const int64_t nc = std::min(chunk, n_cells - c0);
    for (int io = 0; io < 2; ++io)
      for (size_t k = 0; k < N[io]; ++k) {
        if (tab[io][k].kind == SHARED) continue;
        char* at = !cell[io][k] ? nullptr : device ? (user[io][k] ? user[io][k] + c0 * cell[io][k] : nullptr) : dev[io][k];
        tab[io][k].set(at);
        if (!device && !io && at) HIP_TRY(hipMemcpy(at, user[io][k] + c0 * cell[io][k], nc * cell[io][k], hipMemcpyHostToDevice));
      }
    double* tan = n_tan ? static_cast<double*>(p->buf[B_TANGENT].p) : nullptr;
    v.curv = n_curv ? static_cast<double*>(p->buf[B_CURVATURE].p) : nullptr;
    if (!v.coef)
      if (int rc = expand_chunk(p, ds, c0, nc, st, &v.coef, nullptr, tan, v.curv)) return rc;
    if (tan) *tangents = tan;
    if (load) {
      const hommx_coef_source& l = load->src;
      double* field = static_cast<double*>(p->buf[B_POLAR].p);
      HIP_TRY(hommx::launch_expand_program(program_args(*l.program), l.program->n_params, l.n_fields, l.table, l.weights, l.n_q, p->desc.dim,
                                           program_rows(l, c0), field, nullptr, p->n_el, nc, st));
      *load->slot = field;
    }
    if (int rc = run(nc, chunk, v)) return rc;
    if (device) continue;
    for (size_t k = 0; k < N[1]; ++k)
      if (cell[1][k] && user[1][k]) HIP_TRY(hipMemcpy(user[1][k] + c0 * cell[1][k], dev[1][k], nc * cell[1][k], hipMemcpyDeviceToHost));
  }
  return HOMMX_OK;
}

// what opens both entry points of a family that takes a source and an argument struct: the source, the struct, `checks` of the struct
// against the plan's descriptor (open_call), then a route that forms correctors
template <typename Args, typename Checks>
int source_open(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const Args* a, bool device, Checks checks) {
  auto more = [&] {
    if (int rc = coef_check(p, src)) return rc;
    if (!a) return fail(HOMMX_EINVAL, "null arguments");
    return checks();
  };
  if (int rc = open_call(p, n_cells, true, "", device, more); rc != GO) return rc;
  if (int rc = corrector_workspace(p)) return rc;
  return GO;
}

// the blocked workspace of a fused 2D plan whose load solve does not run on its own records (HOMMX_FUSED_LOADS=0 / HOMMX_FUSED_CORR=0)
int load_workspace(hommx_plan* p) {
  if (p->ws || fused_loads(p) || mesh_loads(p)) return HOMMX_OK;
  int rc = hommx::blocked_workspace_create(&p->ws, p->desc.dim, p->desc.n_micro, p->desc.kind);
  return rc ? prefix_error(rc, "blocked path: ") : HOMMX_OK;
}

// -- reconstruction (hommx_reconstruct_batch[_device], hommx_reconstruct_source[_device]) ------------------------------------------------
// the arguments of a reconstruction beside the source and M (these entry points have no public struct); region: the label of every element
struct ReconCall {
  const double* xi;
  int32_t n_regions;
  const uint8_t* region;
  double *stats, *region_stats, *strain, *flux, *A_eff;
  int32_t* info;
};

// one chunk of at most recon_chunk() cells on the device: the correctors into the plan's scratch, then k_recon
int recon_run(hommx_plan* p, int64_t nc, int64_t chunk, const Chunk<ReconCall>& v, hipStream_t st) {
  const bool lds = recon_in_lds(p);
  double *d_A_eff = v.a.A_eff, *corr = nullptr;
  if (int rc = chunk_correctors(p, nc, chunk, v.coef, v.M, &d_A_eff, v.a.info, lds ? 0 : 1, st, &corr)) return rc;
  hommx::ReconArgs a;
  set_geometry(p, a);
  a.corr = corr;
  a.coef = v.coef;
  a.M = v.M;
  a.xi = v.a.xi;
  a.stats = v.a.stats;
  a.strain = v.a.strain;
  a.flux = v.a.flux;
  a.slot = lds ? nullptr : corr + chunk * p->ks.t * a.ndof;
  a.n_regions = v.a.n_regions;
  a.region = !v.a.n_regions ? nullptr : v.a.region ? v.a.region : v.src->mask;  // n_regions == 2 of a two-phase source: the mask may be the labels
  a.region_stats = v.a.region_stats;
  HIP_TRY(hommx::launch_reconstruct(a, nc, st));
  return HOMMX_OK;
}

// the regions of hommx_reconstruct_source[_device]; `s` has passed coef_check
int regions_check(const hommx_coef_source* s, int32_t n_regions, const void* region, const void* region_stats) {
  if (n_regions < 0 || n_regions > HOMMX_RECON_MAX_REGIONS)
    return fail(HOMMX_EINVAL, "n_regions must be 0 .. %d, got %d", HOMMX_RECON_MAX_REGIONS, n_regions);
  const bool mask_labels = s->form == HOMMX_COEF_TWO_PHASE && n_regions == 2 && !region;
  if (n_regions == 0 ? (region || region_stats) : (!region_stats || (!region && !mask_labels)))
    return fail(HOMMX_EINVAL, "region and region_stats: both with n_regions > 0 (n_regions == 2 of a two-phase source: the mask may be "
                              "the labels), neither with n_regions == 0");
  return HOMMX_OK;
}

// the shared argument checks of the reconstruct entry points; `more`: the source and the regions of the entry points that take them
template <typename More>
int recon_open(hommx_plan* p, int64_t n_cells, const void* coef, const ReconCall& a, bool device, More more) {
  if (int rc = open_call(p, n_cells, coef && a.xi && a.stats, "coef / xi / stats", device, more); rc != GO) return rc;
  if (!a.strain != !a.flux) return fail(HOMMX_EINVAL, "strain and flux: both or neither");
  if (int rc = corrector_workspace(p)) return rc;  // a reconstruction needs a route that forms correctors
  return GO;
}

int recon_call(hommx_plan* p, int64_t n_cells, const hommx_coef_source& s, const double* M, const ReconCall& args, bool device, hipStream_t st) {
  const int64_t t = p->ks.t, field = p->n_el * t;
  Chunk<ReconCall> v{};
  ReconCall& a = v.a = args;
  const CellArray in[] = {{&a.xi, t}, {&a.region, p->n_el, SHARED, sizeof(uint8_t)}};
  const CellArray out[] = {{&a.stats, HOMMX_RECON_NSTATS(t)},
                           {&a.A_eff, t * t, KEPT},
                           {&a.strain, field},
                           {&a.flux, field},
                           {&a.region_stats, a.n_regions * HOMMX_RECON_NREGION(t)}};
  return derived_call(p, n_cells, s, M, v, in, out, &a.info, 0, recon_chunk, device, st,
                      [&](int64_t nc, int64_t chunk, const Chunk<ReconCall>& c) { return recon_run(p, nc, chunk, c, st); });
}

// -- sensitivities (hommx_sensitivity_source[_device]) -----------------------------------------------------------------------------------
// the arguments of k_sens for the first derivatives along the directions of a chunk
hommx::SensArgs sens_dirs_args(const hommx_plan* p, const double* corr, const double* M, int32_t n_dirs, int32_t per_cell, const double* dirs,
                               double* dA) {
  hommx::SensArgs k;
  set_geometry(p, k);
  k.corr = corr;
  k.M = M;
  k.n_dirs = n_dirs;
  k.per_cell = per_cell != 0;
  k.dirs = dirs;
  k.dA = dA;
  return k;
}

// one chunk of at most recon_chunk() cells on the device: the correctors into the plan's scratch, then k_sens
int sens_run(hommx_plan* p, int64_t nc, int64_t chunk, const Chunk<hommx_sens_args>& v, hipStream_t st) {
  const hommx_sens_args& a = v.a;
  double *d_A_eff = a.A_eff, *corr = nullptr;
  if (int rc = chunk_correctors(p, nc, chunk, v.coef, v.M, &d_A_eff, a.info, 0, st, &corr)) return rc;
  hommx::SensArgs k = sens_dirs_args(p, corr, v.M, a.n_dirs, a.per_cell, a.dirs, a.dA);
  k.weights = a.weights;
  k.grad = a.grad;
  HIP_TRY(hommx::launch_sensitivity(k, nc, st));
  return HOMMX_OK;
}

// HOMMX_DIRS_PARAMETERS: the directions are the parameter tangents of the source's program; `s` has passed coef_check.
// HOMMX_DIRS_PARAMETERS_CURVATURE (hommx_sens2_args only): the same, and d2A also takes dA_H along the second-order streams
bool curvature_dirs(int32_t per_cell) { return per_cell == HOMMX_DIRS_PARAMETERS_CURVATURE; }
bool parameter_dirs(int32_t per_cell) { return per_cell == HOMMX_DIRS_PARAMETERS || curvature_dirs(per_cell); }
int parameter_dirs_check(const hommx_coef_source* s, int32_t n_dirs, const void* dirs) {
  if (s->form != HOMMX_COEF_PROGRAM) return fail(HOMMX_EINVAL, "HOMMX_DIRS_PARAMETERS needs a HOMMX_COEF_PROGRAM source, got form %d", s->form);
  if (int rc = tangent_slots_check(s, "HOMMX_DIRS_PARAMETERS")) return rc;
  if (s->n_fields == 0 && n_dirs != s->program->n_params)
    return fail(HOMMX_EINVAL, "HOMMX_DIRS_PARAMETERS: n_dirs must be the program's n_params (%d), got %d", s->program->n_params, n_dirs);
  if (n_dirs != s->program->n_params + s->n_fields)
    return fail(HOMMX_EINVAL, "HOMMX_DIRS_PARAMETERS: n_dirs must be the source's n_params (%d) + n_fields (%d), got %d", s->program->n_params,
                s->n_fields, n_dirs);
  if (dirs) return fail(HOMMX_EINVAL, "HOMMX_DIRS_PARAMETERS: dirs must be NULL (the library forms the directions)");
  return HOMMX_OK;
}

int sens_checks(const hommx_coef_source* s, const hommx_sens_args* a) {
  if (a->n_dirs < 0 || a->n_dirs > HOMMX_SENS_MAX_DIRS)
    return fail(HOMMX_EINVAL, "n_dirs must be 0 .. %d, got %d", HOMMX_SENS_MAX_DIRS, a->n_dirs);
  if (curvature_dirs(a->per_cell))
    return fail(HOMMX_EINVAL, "HOMMX_DIRS_PARAMETERS_CURVATURE is a value of per_cell in hommx_sens2_args only: first derivatives have no "
                              "curvature term (use HOMMX_DIRS_PARAMETERS)");
  if (parameter_dirs(a->per_cell))
    if (int rc = parameter_dirs_check(s, a->n_dirs, a->dirs)) return rc;
  if (a->n_dirs > 0 && !((a->dirs || parameter_dirs(a->per_cell)) && a->dA)) return fail(HOMMX_EINVAL, "n_dirs > 0 needs both dirs and dA");
  if (!a->weights != !a->grad) return fail(HOMMX_EINVAL, "weights and grad: both or neither");
  if (a->n_dirs == 0 && !a->grad) return fail(HOMMX_EINVAL, "nothing requested: neither directions nor a gradient");
  return HOMMX_OK;
}

int sens_call(hommx_plan* p, int64_t n_cells, const hommx_coef_source& s, const double* M, const hommx_sens_args& args, bool device,
              hipStream_t st) {
  const int64_t tt = p->ks.t * p->ks.t, el = p->n_el * p->ks.n_comp;
  Chunk<hommx_sens_args> v{};
  hommx_sens_args& a = v.a = args;
  const CellArray in[] = {{&a.dirs, a.n_dirs * el, a.n_dirs && a.per_cell ? PER_CELL : SHARED}, {&a.weights, tt}};
  const CellArray out[] = {{&a.dA, a.n_dirs * tt}, {&a.A_eff, tt, KEPT}, {&a.grad, el}};
  return derived_call(p, n_cells, s, M, v, in, out, &a.info, 0, recon_chunk, device, st,
                      [&](int64_t nc, int64_t chunk, const Chunk<hommx_sens_args>& c) { return sens_run(p, nc, chunk, c, st); },
                      parameter_dirs(a.per_cell) ? &a.dirs : nullptr);
}

// -- stratification sensitivities (hommx_stratification_sensitivity_source[_device]) --------------------------------------------------------
// one chunk of at most recon_chunk() cells on the device: the correctors into the plan's scratch, then k_sens_strat
int strat_run(hommx_plan* p, int64_t nc, int64_t chunk, const Chunk<hommx_strat_sens_args>& v, hipStream_t st) {
  double *d_A_eff = v.a.A_eff, *corr = nullptr;
  if (int rc = chunk_correctors(p, nc, chunk, v.coef, v.M, &d_A_eff, v.a.info, 0, st, &corr)) return rc;
  hommx::StratSensArgs k;
  set_geometry(p, k);
  k.corr = corr;
  k.coef = v.coef;
  k.M = v.M;
  k.dA_dM = v.a.dA_dM;
  k.weights = v.a.weights;
  k.grad_M = v.a.grad_M;
  HIP_TRY(hommx::launch_sens_strat(k, nc, st));
  return HOMMX_OK;
}

int strat_checks(const hommx_strat_sens_args* a) {
  if (!a->weights != !a->grad_M) return fail(HOMMX_EINVAL, "weights and grad_M: both or neither");
  if (!a->dA_dM && !a->grad_M) return fail(HOMMX_EINVAL, "nothing requested: neither dA_dM nor grad_M");
  return HOMMX_OK;
}

int strat_call(hommx_plan* p, int64_t n_cells, const hommx_coef_source& s, const double* M, const hommx_strat_sens_args& args, bool device,
               hipStream_t st) {
  const int64_t dd = p->desc.dim * p->desc.dim, tt = p->ks.t * p->ks.t;
  Chunk<hommx_strat_sens_args> v{};
  hommx_strat_sens_args& a = v.a = args;
  const CellArray in[] = {{&a.weights, tt}};
  const CellArray out[] = {{&a.dA_dM, dd * tt}, {&a.A_eff, tt, KEPT}, {&a.grad_M, dd}};
  return derived_call(p, n_cells, s, M, v, in, out, &a.info, 0, recon_chunk, device, st,
                      [&](int64_t nc, int64_t chunk, const Chunk<hommx_strat_sens_args>& c) { return strat_run(p, nc, chunk, c, st); });
}

// -- polarisation loads (hommx_loads_source[_device]) ------------------------------------------------------------------------------------
bool load_response(const hommx_load_args& a) { return a.energy || a.stats || a.strain || a.flux || a.correctors; }
// the code in hommx_load_args.per_cell: where the load comes from (HOMMX_LOADS_SHARED / _PER_CELL / _PROGRAM), and whether it is an eigenstrain
int load_form(int32_t code) { return code & 3; }
bool load_eigenstrain(int32_t code) { return (code & HOMMX_LOADS_EIGENSTRAIN) != 0; }
// a caller's arguments that loads_open has passed: P_source, the member a caller built against the shorter struct does not have, is
// read for its own code only
hommx_load_args load_args_of(const hommx_load_args& a) {
  hommx_load_args c{};
  c.n_loads = a.n_loads;
  c.per_cell = a.per_cell;
  c.P = load_form(a.per_cell) == HOMMX_LOADS_PROGRAM ? nullptr : a.P;
  c.P_eff = a.P_eff;
  c.A_eff = a.A_eff;
  c.energy = a.energy;
  c.stats = a.stats;
  c.strain = a.strain;
  c.flux = a.flux;
  c.correctors = a.correctors;
  c.info = a.info;
  c.P_source = load_form(a.per_cell) == HOMMX_LOADS_PROGRAM ? a.P_source : nullptr;
  return c;
}
// an eigenstrain array the plan must not overwrite: one that every cell shares, and in a device call the caller's own per-cell array
// (a host call's per-cell array lies in B_IN, the expansion of a program in B_POLAR: those become the eigenstress in place)
bool eigenstress_scratch(int32_t code, bool device) {
  return load_eigenstrain(code) && (load_form(code) == HOMMX_LOADS_SHARED || (load_form(code) == HOMMX_LOADS_PER_CELL && device));
}

// The correctors of the loads `lo` of nc cells of a chunk into corr_l[nc][t][ndof] (rows l < n_loads), on the route
// hommx_plan_load_kernel_name names: fused 2D plans substitute on the records the canonical pass of this chunk has just left in B_FACT
// (k_fused2d_subst_rhs), flagged frontal mesh plans on the pivot columns it has left in the arena (k_mesh_front_rhs; load_chunk keeps
// them resident), flagged plans of the tree routes on the fronts it has left in the corrector plan's arena (mf_load_correctors); every
// other plan runs a corrector pass of the blocked family on the overridden load rows
int load_correctors(hommx_plan* p, int64_t nc, int64_t chunk, const double* d_coef, const double* d_M, const hommx::LoadOverride& lo, hipStream_t st,
                    double* corr_l) {
  if (fused_loads(p)) {
    HIP_TRY(hommx::launch_fused2d_subst_rhs(static_cast<const double*>(p->buf[B_FACT].p), lo.P, lo.n_loads, lo.per_cell, d_M, corr_l,
                                            p->desc.n_micro, nc, st));
    return HOMMX_OK;
  }
  if (mesh_loads(p)) {
    const int rc = hommx::mesh_load_correctors(p->mesh, nc, lo, d_M, corr_l, st);
    return rc ? route_fail(p, rc) : HOMMX_OK;
  }
  if (tree_loads(p)) {
    const int rc = hommx::blocked_load_correctors(p->ws, nc, lo, d_M, corr_l, st);
    return rc ? prefix_error(rc, p->desc.n_micro ? "multifrontal_subst: " : "mesh_multifrontal_subst: ") : HOMMX_OK;
  }
  const int t = p->ks.t;
  if (int rc = grow(p->buf[B_LOADS], sizeof(double) * chunk * t * t)) return rc;
  if (int rc = hommx::blocked_solve(p->ws, nc, d_coef, d_M, static_cast<double*>(p->buf[B_LOADS].p), nullptr, st, corr_l, &lo)) return route_fail(p, rc);
  return HOMMX_OK;
}

// one chunk of at most recon_chunk() cells on the device: the canonical correctors into the plan's scratch and k_polar; for a response
// the correctors of the loads behind them (load_correctors) and k_load_stats
// an eigenstrain first becomes the eigenstress of every cell (k_eigenstress: in place, or into B_POLAR where the array is not the plan's
// to overwrite), which every consumer then reads as a per-cell load
int loads_run(hommx_plan* p, int64_t nc, int64_t chunk, const Chunk<hommx_load_args>& v, bool device, hipStream_t st) {
  const hommx_load_args& a = v.a;
  const bool response = load_response(a);
  const int t = p->ks.t;
  const double* P = a.P;
  bool per_cell = load_form(a.per_cell) != HOMMX_LOADS_SHARED;
  if (load_eigenstrain(a.per_cell)) {
    double* stress = const_cast<double*>(a.P);
    if (eigenstress_scratch(a.per_cell, device)) {
      if (int rc = grow(p->buf[B_POLAR], sizeof(double) * chunk * a.n_loads * p->n_el * t)) return rc;
      stress = static_cast<double*>(p->buf[B_POLAR].p);
    }
    HIP_TRY(hommx::launch_eigenstress(p->desc.dim, p->desc.kind, v.coef, a.P, per_cell, stress, a.n_loads, p->n_el, nc, st));
    P = stress;
    per_cell = true;
  }
  double *d_A_eff = a.A_eff, *corr = nullptr;
  if (int rc = chunk_correctors(p, nc, chunk, v.coef, v.M, &d_A_eff, a.info, response ? t : 0, st, &corr)) return rc;
  hommx::LoadArgs k;
  set_geometry(p, k);
  k.corr = corr;
  k.coef = v.coef;
  k.M = v.M;
  k.n_loads = a.n_loads;
  k.per_cell = per_cell;
  k.P = P;
  k.P_eff = a.P_eff;
  HIP_TRY(hommx::launch_polar(k, nc, st));
  if (!response) return HOMMX_OK;
  double* corr_l = corr + chunk * t * k.ndof;
  if (int rc = load_correctors(p, nc, chunk, v.coef, v.M, hommx::LoadOverride{P, a.n_loads, per_cell}, st, corr_l)) return rc;
  k.corr = corr_l;
  k.energy = a.energy;
  k.stats = a.stats;
  k.strain = a.strain;
  k.flux = a.flux;
  if (a.energy || a.stats || a.strain) HIP_TRY(hommx::launch_load_stats(k, nc, st));
  if (a.correctors)  // rows l < n_loads of every cell
    HIP_TRY(hipMemcpy2DAsync(a.correctors, sizeof(double) * a.n_loads * k.ndof, corr_l, sizeof(double) * t * k.ndof,
                             sizeof(double) * a.n_loads * k.ndof, nc, hipMemcpyDeviceToDevice, st));
  return HOMMX_OK;
}

// the code of a load (hommx_load_args.per_cell; hommx_criterion_args.per_cell) and, for HOMMX_LOADS_PROGRAM, its source `l`
int load_code_check(const hommx_plan* p, int32_t n_loads, int32_t code, const hommx_coef_source* l) {
  if ((code & ~7) || load_form(code) == 3)
    return fail(HOMMX_EINVAL, "unknown load code %d in per_cell: HOMMX_LOADS_SHARED, HOMMX_LOADS_PER_CELL or HOMMX_LOADS_PROGRAM, alone or "
                              "or-ed with HOMMX_LOADS_EIGENSTRAIN", code);
  if (load_form(code) != HOMMX_LOADS_PROGRAM) return HOMMX_OK;
  if (!l) return fail(HOMMX_EINVAL, "HOMMX_LOADS_PROGRAM needs P_source, the program source of the load");
  if (l->form != HOMMX_COEF_PROGRAM) return fail(HOMMX_EINVAL, "P_source must be a HOMMX_COEF_PROGRAM source, got form %d", l->form);
  if (n_loads != 1) return fail(HOMMX_EINVAL, "HOMMX_LOADS_PROGRAM takes n_loads == 1 (callers loop for more), got %d", n_loads);
  if (int rc = program_check(p, l, hommx::kind_sizes(p->desc.dim, p->desc.kind).t)) return prefix_error(rc, "P_source: ");
  return HOMMX_OK;
}

// what refuses a load solve before any work: the one check that reads more of the plan than its descriptor (its family), so it cannot
// run on the plan-shaped memory the argument checks accept: it comes after open_call, with the device current already
int load_solve_check(const hommx_plan* p) {
  if (p->family == FAM_MESH && !mesh_loads(p))
    return fail(HOMMX_EINVAL, "the frontal mesh route (mesh_front) solves for the canonical loads only: energy, stats, strain / flux and "
                              "correctors of user loads need a plan of the tree route (HOMMX_MESH_FLAG_TREE, route=\"tree\"); P_eff alone works here");
  return HOMMX_OK;
}

// the argument checks of both entry points, then the routes the call needs: one that forms correctors, and for a response a load solve
int loads_open(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const hommx_load_args* a, bool device) {
  auto checks = [&] {
    const int t = hommx::kind_sizes(p->desc.dim, p->desc.kind).t;
    if (a->n_loads < 1 || a->n_loads > t) return fail(HOMMX_EINVAL, "n_loads must be 1 .. %d (the tensor size of the plan), got %d", t, a->n_loads);
    if (int rc = load_code_check(p, a->n_loads, a->per_cell, a->P_source)) return rc;
    if (load_form(a->per_cell) == HOMMX_LOADS_PROGRAM) {
      if (!a->P_eff) return fail(HOMMX_EINVAL, "null P_eff");
    } else if (!a->P || !a->P_eff) {
      return fail(HOMMX_EINVAL, "null P / P_eff");
    }
    if (!a->strain != !a->flux) return fail(HOMMX_EINVAL, "strain and flux: both or neither");
    return HOMMX_OK;
  };
  if (int rc = source_open(p, n_cells, src, a, device, checks); rc != GO) return rc;
  if (!load_response(*a)) return GO;
  if (int rc = load_solve_check(p)) return rc;  // before any work (a mesh plan gets no workspace above)
  if (int rc = load_workspace(p)) return rc;
  return GO;
}

// A response holds a second corrector block per cell, and its chunks end in a load solve
int loads_call(hommx_plan* p, int64_t n_cells, const hommx_coef_source& s, const double* M, const hommx_load_args& args, bool device,
               hipStream_t st) {
  const int64_t t = p->ks.t, nl = args.n_loads, field = nl * p->n_el * t;
  const bool response = load_response(args);
  Chunk<hommx_load_args> v{};
  hommx_load_args& a = v.a = load_args_of(args);
  const bool program = load_form(a.per_cell) == HOMMX_LOADS_PROGRAM;
  ProgramLoad load{};
  if (program) {
    const hommx_coef_source& l = *a.P_source;
    load = {program_source(l.program, l.n_q, l.table, l.weights, l.params, l.n_fields), &a.P};
  }
  // what a chunk holds of the load beside the caller's array: the expansion of a program, the eigenstresses of an array that stays as it is
  const size_t formed = program || eigenstress_scratch(a.per_cell, device) ? sizeof(double) * field : 0;
  const CellArray in[] = {{&a.P, field, load_form(a.per_cell) == HOMMX_LOADS_SHARED ? SHARED : PER_CELL}};
  const CellArray out[] = {{&a.P_eff, nl * t}, {&a.A_eff, t * t, KEPT},   {&a.energy, nl * nl},          {&a.stats, nl * (t + 2)},
                           {&a.strain, field}, {&a.flux, field},          {&a.correctors, nl * plan_ndof(p)}};
  return derived_call(p, n_cells, s, M, v, in, out, &a.info, formed + (response ? sizeof(double) * plan_ndof(p) * t : 0),
                      response ? load_chunk : recon_chunk, device, st,
                      [&](int64_t nc, int64_t chunk, const Chunk<hommx_load_args>& c) { return loads_run(p, nc, chunk, c, device, st); },
                      nullptr, false, program ? &load : nullptr);
}

// -- failure criteria (hommx_criterion_source[_device]) ------------------------------------------------------------------------------------
// a caller's arguments that crit_open has passed: the load members are read with has_load only, P_source for its own code only
hommx_criterion_args crit_args_of(const hommx_criterion_args& a) {
  hommx_criterion_args c = a;
  const bool program = a.has_load && load_form(a.per_cell) == HOMMX_LOADS_PROGRAM;
  c.has_load = a.has_load != 0;
  c.per_cell = a.has_load ? a.per_cell : 0;
  c.P = a.has_load && !program ? a.P : nullptr;
  c.P_source = program ? a.P_source : nullptr;
  return c;
}
// the field of a cell lies in LDS beside the stack rows of the program, or in a slot of the chunk's scratch
bool crit_in_lds(const hommx_plan* p, int depth) { return hommx::criterion_lds_bytes(plan_ndof(p), depth) <= hommx::recon_lds_limit(); }

// one chunk on the device.  Without a load: the canonical correctors into the plan's scratch, then k_criterion.  With one, the chunk of
// a response of loads_run: the eigenstress where the flag is set, the canonical correctors, the corrector of the load into the second
// block (load_correctors), then k_criterion with chi_P and P
int crit_run(hommx_plan* p, int64_t nc, int64_t chunk, const Chunk<hommx_criterion_args>& v, bool device, hipStream_t st) {
  const hommx_criterion_args& a = v.a;
  const int t = p->ks.t, depth = program_depth(*a.program);
  const bool slot = !crit_in_lds(p, depth);
  const double* P = a.P;
  if (a.has_load && load_eigenstrain(a.per_cell)) {
    double* stress = const_cast<double*>(a.P);
    if (eigenstress_scratch(a.per_cell, device)) {
      if (int rc = grow(p->buf[B_POLAR], sizeof(double) * chunk * p->n_el * t)) return rc;
      stress = static_cast<double*>(p->buf[B_POLAR].p);
    }
    HIP_TRY(hommx::launch_eigenstress(p->desc.dim, p->desc.kind, v.coef, a.P, true, stress, 1, p->n_el, nc, st));
    P = stress;
  }
  double *d_A_eff = a.A_eff, *corr = nullptr;
  if (int rc = chunk_correctors(p, nc, chunk, v.coef, v.M, &d_A_eff, a.info, (a.has_load ? t : 0) + (slot ? 1 : 0), st, &corr)) return rc;
  hommx::CritArgs k;
  set_geometry(p, k);
  k.corr = corr;
  k.coef = v.coef;
  k.M = v.M;
  k.xi = a.xi;
  k.prog = program_args(*a.program);
  k.n_fields = a.n_fields;
  k.rows = a.rows;
  k.points = a.points;
  k.threshold = a.threshold;
  k.crit = a.crit;
  k.values = a.values;
  k.strain = a.strain;
  k.flux = a.flux;
  double* behind = corr + chunk * t * k.ndof;
  if (a.has_load) {
    if (int rc = load_correctors(p, nc, chunk, v.coef, v.M, hommx::LoadOverride{P, 1, true}, st, behind)) return rc;
    k.corr_load = behind;
    k.P = P;
    k.per_cell = true;
    behind += chunk * t * k.ndof;
  }
  k.slot = slot ? behind : nullptr;
  HIP_TRY(hommx::launch_criterion(k, depth, nc, st));
  return HOMMX_OK;
}

// the argument checks of both entry points, then the routes the call needs: one that forms correctors, and with a load a load solve
int crit_open(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const hommx_criterion_args* a, bool device) {
  auto checks = [&] {
    const hommx::KindSizes ks = hommx::kind_sizes(p->desc.dim, p->desc.kind);
    if (!a->program) return fail(HOMMX_EINVAL, "null program");
    if (!a->rows || !a->xi || !a->crit) return fail(HOMMX_EINVAL, "null rows / xi / crit");
    if (!a->strain != !a->flux) return fail(HOMMX_EINVAL, "strain and flux: both or neither");
    hommx_coef_source own{};  // what program_check reads of a source
    own.n_fields = a->n_fields;
    own.program = a->program;
    if (int rc = program_check(p, &own, 0, 2 * ks.t + ks.n_comp)) return rc;
    if (!a->points)
      for (int pc = 0; pc < a->program->n_ops; ++pc)
        if (a->program->ops[2 * pc] == hommx::OP_Y)
          return fail(HOMMX_EINVAL, "null points: the program reads y (instruction %d), the centroid of the element", pc);
    if (a->threshold != a->threshold) return fail(HOMMX_EINVAL, "the threshold is NaN");
    if (!a->has_load) return HOMMX_OK;
    if (int rc = load_code_check(p, 1, a->per_cell, a->P_source)) return rc;
    if (load_form(a->per_cell) == HOMMX_LOADS_SHARED)
      return fail(HOMMX_EINVAL, "a criterion takes its load per cell (HOMMX_LOADS_PER_CELL) or as a program (HOMMX_LOADS_PROGRAM): points is "
                                "the one array every cell shares");
    if (load_form(a->per_cell) == HOMMX_LOADS_PER_CELL && !a->P) return fail(HOMMX_EINVAL, "null P");
    return HOMMX_OK;
  };
  if (int rc = source_open(p, n_cells, src, a, device, checks); rc != GO) return rc;
  if (!a->has_load) return GO;
  if (int rc = load_solve_check(p)) return rc;
  if (int rc = load_workspace(p)) return rc;
  return GO;
}

// With a load a chunk holds a second corrector block per cell and ends in a load solve; the slot of a field that does not fit LDS
// beside the stack counts where the chunk rule of the reconstruction does not count one already
int crit_call(hommx_plan* p, int64_t n_cells, const hommx_coef_source& s, const double* M, const hommx_criterion_args& args, bool device,
              hipStream_t st) {
  const int64_t t = p->ks.t, field = p->n_el * t;
  Chunk<hommx_criterion_args> v{};
  hommx_criterion_args& a = v.a = crit_args_of(args);
  const bool program = a.P_source != nullptr;
  ProgramLoad load{};
  if (program) {
    const hommx_coef_source& l = *a.P_source;
    load = {program_source(l.program, l.n_q, l.table, l.weights, l.params, l.n_fields), &a.P};
  }
  const size_t formed = program || (a.has_load && eigenstress_scratch(a.per_cell, device)) ? sizeof(double) * field : 0;
  const bool own_slot = !crit_in_lds(p, program_depth(*a.program)) && recon_in_lds(p);
  const size_t blocks = sizeof(double) * plan_ndof(p) * ((a.has_load ? t : 0) + (own_slot ? 1 : 0));
  const CellArray in[] = {{&a.rows, hommx::program_row_doubles(a.n_fields)},
                          {&a.xi, t},
                          {&a.P, a.has_load ? field : 0},
                          {&a.points, p->n_el * p->desc.dim, SHARED}};
  const CellArray out[] = {{&a.crit, HOMMX_CRIT_NSTATS}, {&a.A_eff, t * t, KEPT}, {&a.values, p->n_el}, {&a.strain, field}, {&a.flux, field}};
  return derived_call(p, n_cells, s, M, v, in, out, &a.info, formed + blocks, a.has_load ? load_chunk : recon_chunk, device, st,
                      [&](int64_t nc, int64_t chunk, const Chunk<hommx_criterion_args>& c) { return crit_run(p, nc, chunk, c, device, st); },
                      nullptr, false, program ? &load : nullptr);
}

// -- the nonlinear family: strain-dependent coefficients (hommx_secant*_source[_device]; DESIGN.md sections 4.15 - 4.19) ------------------
// One request describes a call of any of the fourteen entries: the iteration's arguments and what the entry takes beside them -- the
// tangent's struct (the tangent entries), a history, a load, a state tail.  A part the entry requires (`need`) must be there; any other
// part that is null is absent
enum : unsigned { NEED_HISTORY = 1, NEED_LOAD = 2, NEED_STATE = 4 };
struct SecantRequest {
  const void* given;                         // the entry's own argument struct: `secant` or, of a tangent entry, `tangent`
  const hommx_secant_args* secant;           // the iteration's: the entry's own struct, or the one the tangent's struct points to
  const hommx_secant_tangent_args* tangent;  // null: no tangent tail
  const hommx_history_args* hist;
  const hommx_secant_load_args* load;
  const hommx_secant_state_args* state;
  unsigned need;
};
SecantRequest secant_request(const hommx_secant_args* a, unsigned need = 0, const hommx_history_args* hist = nullptr,
                             const hommx_secant_load_args* load = nullptr, const hommx_secant_state_args* state = nullptr) {
  return {a, a, nullptr, hist, load, state, need};
}
SecantRequest secant_request(const hommx_secant_tangent_args* a, unsigned need = 0, const hommx_history_args* hist = nullptr,
                             const hommx_secant_load_args* load = nullptr) {
  return {a, a ? a->secant : nullptr, a, hist, load, nullptr, need};
}

// The request as the chunk driver re-bases it: a copy of every struct that is there (h.n_history 0 and null pointers: no history).
// l.P is the load array of the chunk, [nc][n_el][t]: the caller's, its copy in B_IN or the expansion of the program in B_POLAR;
// l.P_source and g.secant are not read
struct SecantCall {
  hommx_secant_args s;
  hommx_history_args h;
  bool has_load, has_state, has_tangent;
  hommx_secant_load_args l;
  hommx_secant_state_args t;
  hommx_secant_tangent_args g;
};

// Where the field of a kernel of the call lives: in LDS beside the interpreter's stack, or, where it does not fit there, in the slot of
// global scratch behind the corrector blocks.  The one definition under the scratch a chunk holds and under every launch
enum SecantKernel { K_ROUND, K_TANGENT, K_CRITERION, K_RECON };
bool secant_field_in_slot(const hommx_plan* p, const SecantCall& c, SecantKernel k) {
  const int depth = program_depth(*c.s.program);
  switch (k) {
    case K_ROUND: return !crit_in_lds(p, depth);
    case K_TANGENT:  // the stack rows of the forward mode are (1 + P) wide
      return c.has_tangent &&
             hommx::secant_tangent_lds_bytes(plan_ndof(p), depth, hommx::secant_tangent_slots(p->ks.t, depth)) > hommx::recon_lds_limit();
    case K_CRITERION: return c.has_state && c.t.crit_program && !crit_in_lds(p, program_depth(*c.t.crit_program));
    case K_RECON: return c.has_state && c.t.reconstruct && !recon_in_lds(p);
  }
  return false;
}
bool secant_slot_used(const hommx_plan* p, const SecantCall& c) {
  const SecantKernel all[] = {K_ROUND, K_TANGENT, K_CRITERION, K_RECON};
  return std::any_of(all, all + 4, [&](SecantKernel k) { return secant_field_in_slot(p, c, k); });
}
// ... and where it is addressed: `corr` holds [canonical blocks | with a load, as many for its corrector | slot] per chunk
double* secant_slot(const hommx_plan* p, const SecantCall& c, SecantKernel k, double* corr, int64_t chunk) {
  return secant_field_in_slot(p, c, k) ? corr + chunk * (c.has_load ? 2 : 1) * p->ks.t * plan_ndof(p) : nullptr;
}

int64_t tangent_stream_doubles(const hommx_plan* p) { return p->n_el * (p->ks.t * (p->ks.t + 1) / 2); }

// what the rounds of a chunk leave for the tails: the blocks are those of the last executed round
struct SecantRounds {
  double* cur;      // the stream the iteration stands on
  double* corr;     // the corrector buffer: the canonical blocks, the load's block, the slot
  double* chi;      // the load's block (null: no load)
  const double* P;  // what that block was solved for: the load array or, of an eigenstrain, the eigenstress of the round (null: no load)
  const double* E;  // the eigenstrain (null: none)
  double* tan;      // scratch of the chunk for the tangent stream (null: the caller takes tangent_coef, or no tangent tail)
};

// the arguments of every round of a chunk but the round's own (corr, load, slot, round).  Without a load its SecantHistoryArgs alone is
// launched, without a history its SecantArgs
hommx::SecantLoadArgs secant_round_args(const hommx_plan* p, const Chunk<SecantCall>& v, double* cur, double* cand, int32_t* info) {
  const hommx_secant_args& a = v.a.s;
  hommx::SecantLoadArgs k;
  set_geometry(p, k);
  k.hist_in = v.a.h.history_in;
  k.hist_out = v.a.h.history_out;
  k.n_history = v.a.h.n_history;
  k.base = v.coef;
  k.cur = cur;
  k.cand = cand;
  k.M = v.M;
  k.xi = a.xi;
  k.prog = program_args(*a.program);
  k.n_fields = a.n_fields;
  k.rows = a.rows;
  k.points = a.points;
  k.max_iter = a.max_iter;
  k.tol = a.tol;
  k.relax = a.relax;
  k.info = info;
  k.state = a.state;
  k.mean_flux = a.mean_flux;
  k.law_values = a.law_values;
  k.strain = a.strain;
  k.flux = a.flux;
  return k;
}

// The rounds of one chunk: the current stream starts as coef_start or the base stream; per round the eigenstress of the current stream
// (an eigenstrain: k_eigenstress into scratch of the chunk), the canonical correctors, with a load its corrector into the block behind
// them (load_correctors: the block layout of crit_run), then k_secant_load, k_secant_history or k_secant_update.  The device entry
// queues max_iter rounds and reads nothing; the host entry reads the chunk's state after each round and stops when no cell runs -- a
// stopped cell is frozen, so the bits are the same
int secant_rounds(hommx_plan* p, int64_t nc, int64_t chunk, const Chunk<SecantCall>& v, bool device, hipStream_t st, SecantRounds* out) {
  const hommx_secant_args& a = v.a.s;
  const int t = p->ks.t, depth = program_depth(*a.program);
  const bool load = v.a.has_load, eigen = load && load_eigenstrain(v.a.l.per_cell);
  const size_t stream = sizeof(double) * p->n_el * p->ks.n_comp;
  const size_t bytes[5] = {stream * chunk, stream * chunk, a.info ? 0 : sizeof(int32_t) * chunk,
                           v.a.has_tangent && !v.a.g.tangent_coef ? sizeof(double) * tangent_stream_doubles(p) * chunk : 0,
                           eigen ? sizeof(double) * p->n_el * t * chunk : 0};
  char* at[5];
  if (int rc = carve(p->buf[B_SECANT], bytes, at)) return rc;
  double *cur = reinterpret_cast<double*>(at[0]), *stress = reinterpret_cast<double*>(at[4]);  // stress: the eigenstress of the round
  int32_t* info = a.info ? a.info : reinterpret_cast<int32_t*>(at[2]);
  HIP_TRY(hipMemcpyAsync(cur, a.coef_start ? a.coef_start : v.coef, stream * nc, hipMemcpyDeviceToDevice, st));
  hommx::SecantLoadArgs k = secant_round_args(p, v, cur, reinterpret_cast<double*>(at[1]), info);
  *out = SecantRounds{cur, nullptr, nullptr, nullptr, eigen ? v.a.l.P : nullptr, reinterpret_cast<double*>(at[3])};
  std::vector<double> seen;
  for (int j = 0; j < a.max_iter; ++j) {
    double* d_A_eff = a.A_eff;
    if (eigen) HIP_TRY(hommx::launch_eigenstress(p->desc.dim, p->desc.kind, cur, v.a.l.P, true, stress, 1, p->n_el, nc, st));
    if (int rc = chunk_correctors(p, nc, chunk, cur, v.M, &d_A_eff, info, (load ? t : 0) + (secant_slot_used(p, v.a) ? 1 : 0), st, &out->corr))
      return rc;
    k.corr = out->corr;
    if (load) {
      out->chi = out->corr + chunk * t * k.ndof;
      out->P = eigen ? stress : v.a.l.P;
      if (int rc = load_correctors(p, nc, chunk, cur, v.M, hommx::LoadOverride{out->P, 1, true}, st, out->chi)) return rc;
      k.load = hommx::RoundLoad{out->chi, eigen ? nullptr : out->P, out->E};
    }
    k.slot = secant_slot(p, v.a, K_ROUND, out->corr, chunk);
    k.round = j;
    HIP_TRY(load          ? hommx::launch_secant_load(k, depth, nc, st)
            : k.n_history ? hommx::launch_secant_history(k, depth, nc, st)
                          : hommx::launch_secant(k, depth, nc, st));
    if (device) continue;
    seen.resize(HOMMX_SECANT_NSTATE * nc);
    HIP_TRY(hipMemcpy(seen.data(), a.state, sizeof(double) * seen.size(), hipMemcpyDeviceToHost));
    bool running = false;
    for (int64_t c = 0; c < nc; ++c) running |= seen[HOMMX_SECANT_NSTATE * c + 2] == -1.0;
    if (!running) break;
  }
  if (a.coef_out) HIP_TRY(hipMemcpyAsync(a.coef_out, cur, stream * nc, hipMemcpyDeviceToDevice, st));
  return HOMMX_OK;
}

// the state tail (hommx_secant_state_source): k_criterion_state and / or k_recon on `cur`, the corrector blocks
// of the last executed round and its load array or eigenstress; no elimination
hommx::CritStateArgs state_criterion_args(const hommx_plan* p, int64_t chunk, const Chunk<SecantCall>& v, const SecantRounds& r) {
  const hommx_secant_state_args& s = v.a.t;
  hommx::CritStateArgs c;
  set_geometry(p, c);
  c.corr = r.corr;
  c.coef = r.cur;
  c.M = v.M;
  c.xi = v.a.s.xi;
  c.prog = program_args(*s.crit_program);
  c.n_fields = s.crit_n_fields;
  c.rows = s.crit_rows;
  c.points = v.a.s.points;
  c.threshold = s.threshold;
  c.crit = s.crit;
  c.values = s.crit_values;
  c.strain = s.total_strain;
  c.flux = s.total_flux;
  c.corr_load = r.chi;
  c.P = r.P;
  c.per_cell = v.a.has_load;
  c.base = v.coef;
  c.hist_in = v.a.h.history_in;
  c.n_history = v.a.h.n_history;
  c.slot = secant_slot(p, v.a, K_CRITERION, r.corr, chunk);
  return c;
}
hommx::ReconArgs state_recon_args(const hommx_plan* p, int64_t chunk, const Chunk<SecantCall>& v, const SecantRounds& r) {
  const hommx_secant_state_args& s = v.a.t;
  hommx::ReconArgs a;
  set_geometry(p, a);
  a.corr = r.corr;
  a.coef = r.cur;
  a.M = v.M;
  a.xi = v.a.s.xi;
  a.stats = s.stats;
  a.slot = secant_slot(p, v.a, K_RECON, r.corr, chunk);
  a.n_regions = s.n_regions;
  a.region = s.n_regions ? s.region : nullptr;
  a.region_stats = s.region_stats;
  return a;
}
int state_tail(hommx_plan* p, int64_t nc, int64_t chunk, const Chunk<SecantCall>& v, const SecantRounds& r, hipStream_t st) {
  if (v.a.t.crit_program)
    HIP_TRY(hommx::launch_criterion_state(state_criterion_args(p, chunk, v, r), program_depth(*v.a.t.crit_program), nc, st));
  if (v.a.t.reconstruct) HIP_TRY(hommx::launch_reconstruct(state_recon_args(p, chunk, v, r), nc, st));
  return HOMMX_OK;
}

// the tangent tail (hommx_secant_tangent_source).  After the last queued round the corrector buffer holds the
// correctors of `cur` for every cell -- a stopped cell's elimination reproduces, a stopping round never commits --, so one launch of
// k_secant_tangent[_history | _load] forms the tangent stream, solve_source_device eliminates it on the tangent plan, in that plan's
// own workspace, and the cells of status 2 or 3 get NaN.  Of the argument struct the base of the kernel that is launched is read, as in a round
hommx::SecantTangentLoadArgs tangent_args(const hommx_plan* p, int64_t chunk, const Chunk<SecantCall>& v, const SecantRounds& r) {
  const hommx_secant_args& a = v.a.s;
  hommx::SecantTangentLoadArgs g;
  set_geometry(p, g);
  g.corr = r.corr;
  g.M = v.M;
  g.base = v.coef;
  g.cur = r.cur;
  g.xi = a.xi;
  g.prog = program_args(*a.program);
  g.n_fields = a.n_fields;
  g.rows = a.rows;
  g.points = a.points;
  g.state = a.state;
  g.tan = v.a.g.tangent_coef ? v.a.g.tangent_coef : r.tan;
  g.asym = v.a.g.asymmetry;
  g.slot = secant_slot(p, v.a, K_TANGENT, r.corr, chunk);
  g.corr_load = r.chi;
  g.E = r.E;
  g.hist_in = v.a.h.history_in;
  g.n_history = v.a.h.n_history;
  if (g.n_history)
    for (int pc = 0; pc < a.program->n_ops; ++pc)  // the updates stand behind the last component's STORE
      if (a.program->ops[2 * pc] == hommx::OP_STORE && a.program->ops[2 * pc + 1] < p->ks.n_comp) g.prog.n_ops = pc + 1;
  return g;
}
int tangent_tail(hommx_plan* p, int64_t nc, int64_t chunk, const Chunk<SecantCall>& v, const SecantRounds& r, hipStream_t st) {
  const hommx::SecantTangentLoadArgs g = tangent_args(p, chunk, v, r);
  const int depth = program_depth(*v.a.s.program);
  HIP_TRY(v.a.has_load  ? hommx::launch_secant_tangent_load(g, depth, nc, st)
          : g.n_history ? hommx::launch_secant_tangent_history(g, depth, nc, st)
                        : hommx::launch_secant_tangent(g, depth, nc, st));
  if (int rc = solve_source_device(v.a.g.tangent_plan, nc, sampled_source(g.tan), v.M, v.a.g.tangent, v.a.g.tangent_info, st)) return rc;
  HIP_TRY(hommx::launch_tangent_mask(v.a.s.state, v.a.g.tangent, p->ks.t * p->ks.t, nc, st));
  return HOMMX_OK;
}

// one chunk on the device: the rounds, then the tails the call has on what the rounds left
int secant_run(hommx_plan* p, int64_t nc, int64_t chunk, const Chunk<SecantCall>& v, bool device, hipStream_t st) {
  SecantRounds r;
  if (int rc = secant_rounds(p, nc, chunk, v, device, st, &r)) return rc;
  if (v.a.has_state)
    if (int rc = state_tail(p, nc, chunk, v, r, st)) return rc;
  return v.a.has_tangent ? tangent_tail(p, nc, chunk, v, r, st) : HOMMX_OK;
}

// the checks of a history struct, then of hommx_secant_args, against the plan's descriptor: the program of a call with a history has
// n_history more components on a row as much longer
int secant_checks(const hommx_plan* p, const SecantRequest& r) {
  const hommx_secant_args* a = r.secant;
  int n_history = 0;
  if (r.hist || (r.need & NEED_HISTORY)) {
    const hommx_history_args* h = r.hist;
    if (!h) return fail(HOMMX_EINVAL, "null history arguments");
    if (h->n_history < 1 || h->n_history > HOMMX_SECANT_MAX_HISTORY)
      return fail(HOMMX_EINVAL, "n_history must be 1 .. %d, got %d", HOMMX_SECANT_MAX_HISTORY, h->n_history);
    if (!h->history_in || !h->history_out) return fail(HOMMX_EINVAL, "null history_in / history_out");
    if (h->history_in == h->history_out)
      return fail(HOMMX_EINVAL, "history_in and history_out are the same array: the input is read in every round");
    n_history = h->n_history;
  }
  const hommx::KindSizes ks = hommx::kind_sizes(p->desc.dim, p->desc.kind);
  if (!a->program) return fail(HOMMX_EINVAL, "null program");
  if (!a->rows || !a->xi || !a->state || !a->A_eff) return fail(HOMMX_EINVAL, "null rows / xi / state / A_eff");
  if (!a->strain != !a->flux) return fail(HOMMX_EINVAL, "strain and flux: both or neither");
  hommx_coef_source own{};  // what program_check reads of a source
  own.n_fields = a->n_fields;
  own.program = a->program;
  if (int rc = program_check(p, &own, 0, 2 * ks.t + ks.n_comp + n_history, ks.n_comp + n_history)) return rc;
  if (!a->points)
    for (int pc = 0; pc < a->program->n_ops; ++pc)
      if (a->program->ops[2 * pc] == hommx::OP_Y)
        return fail(HOMMX_EINVAL, "null points: the program reads y (instruction %d), the centroid of the element", pc);
  if (a->max_iter < 1) return fail(HOMMX_EINVAL, "max_iter must be at least 1, got %d", a->max_iter);
  if (!(a->tol >= 0.0)) return fail(HOMMX_EINVAL, "tol must be a number >= 0, got %g", a->tol);
  if (!(a->relax > 0.0 && a->relax <= 1.0)) return fail(HOMMX_EINVAL, "relax must lie in (0, 1], got %g", a->relax);
  return HOMMX_OK;
}

// the load (hommx_secant_load_args) against the plan's descriptor
int secant_load_checks(const hommx_plan* p, const hommx_secant_load_args* l) {
  if (!l) return fail(HOMMX_EINVAL, "null load arguments");
  if (int rc = load_code_check(p, 1, l->per_cell, l->P_source)) return rc;
  if (load_form(l->per_cell) == HOMMX_LOADS_SHARED)
    return fail(HOMMX_EINVAL, "a law takes its load per cell (HOMMX_LOADS_PER_CELL) or as a program (HOMMX_LOADS_PROGRAM): points is the "
                              "one array every cell shares");
  if (load_form(l->per_cell) == HOMMX_LOADS_PER_CELL && !l->P) return fail(HOMMX_EINVAL, "null P");
  return HOMMX_OK;
}

// what a call with a load needs beside a route that forms correctors: a load solve, as crit_open
int secant_load_routes(hommx_plan* p) {
  if (int rc = load_solve_check(p)) return rc;
  if (int rc = load_workspace(p)) return rc;
  return GO;
}

// the tangent's own arguments against the descriptors of both plans alone (of a mesh plan, whose descriptor has no size, the element
// and node counts as well); the iteration's have passed secant_checks
int secant_tangent_checks(const hommx_plan* p, const hommx_secant_tangent_args* a) {
  const hommx_secant_args& s = *a->secant;
  const hommx::KindSizes ks = hommx::kind_sizes(p->desc.dim, p->desc.kind);
  if (!a->tangent_plan || !a->tangent || !a->asymmetry) return fail(HOMMX_EINVAL, "null tangent_plan / tangent / asymmetry");
  const hommx_plan* q = a->tangent_plan;
  if (q == p) return fail(HOMMX_EINVAL, "tangent_plan is the plan itself: the tangent elimination needs a plan of its own");
  const int want = hommx::tangent_kind(p->desc.kind);
  if (q->desc.kind != want)
    return fail(HOMMX_EINVAL, "tangent_plan has kind %d; the tangent kind of a plan of kind %d is %d", q->desc.kind, p->desc.kind, want);
  if (q->desc.dim != p->desc.dim) return fail(HOMMX_EINVAL, "tangent_plan has dim %d; the plan has %d", q->desc.dim, p->desc.dim);
  if (q->desc.n_micro != p->desc.n_micro)
    return fail(HOMMX_EINVAL, "tangent_plan has n_micro %d; the plan has %d", q->desc.n_micro, p->desc.n_micro);
  if (q->desc.device != p->desc.device)
    return fail(HOMMX_EINVAL, "tangent_plan is on device %d; the plan on %d", q->desc.device, p->desc.device);
  if (p->desc.n_micro == 0 && (q->n_el != p->n_el || plan_ndof(q) / q->ks.bs != plan_ndof(p) / p->ks.bs))
    return fail(HOMMX_EINVAL, "tangent_plan is a plan of another mesh: %lld elements, the plan has %lld", (long long)q->n_el,
                (long long)p->n_el);
  const int lo = hommx::program_row_doubles(s.n_fields) + ks.t;
  for (int pc = 0; pc < s.program->n_ops; ++pc) {
    const int op = s.program->ops[2 * pc], k = s.program->ops[2 * pc + 1];
    if (op == hommx::OP_X && k >= lo && k < lo + ks.t)
      return fail(HOMMX_EINVAL, "the law reads s[%d] (instruction %d): the consistent tangent takes an explicit law, one that reads no "
                                "s[k]; an implicit law is out of scope", k - lo, pc);
  }
  return HOMMX_OK;
}

// the tail of hommx_secant_state_source against the plan's descriptor: the criterion as crit_open checks
// one, on the row of a state criterion; the reconstruction as recon_open checks its regions.  The other parts of the request have
// passed their own checks
int secant_state_checks(const hommx_plan* p, const hommx_coef_source* src, const SecantRequest& r) {
  const hommx_secant_state_args* s = r.state;
  if (!s) return fail(HOMMX_EINVAL, "null state arguments");
  if (!s->crit_program && !s->reconstruct) return fail(HOMMX_EINVAL, "nothing requested: neither a criterion nor the reconstruction");
  const hommx::KindSizes ks = hommx::kind_sizes(p->desc.dim, p->desc.kind);
  if (s->crit_program) {
    if (!s->crit_rows || !s->crit) return fail(HOMMX_EINVAL, "null crit_rows / crit");
    if (!s->total_strain != !s->total_flux) return fail(HOMMX_EINVAL, "total_strain and total_flux: both or neither");
    hommx_coef_source own{};  // what program_check reads of a source
    own.n_fields = s->crit_n_fields;
    own.program = s->crit_program;
    // without a history struct the row ends behind the two coefficient segments: an h index of the criterion is out of range
    if (int rc = program_check(p, &own, 0, 2 * ks.t + 2 * ks.n_comp + (r.hist ? r.hist->n_history : 0))) return rc;
    if (!r.secant->points)
      for (int pc = 0; pc < s->crit_program->n_ops; ++pc)
        if (s->crit_program->ops[2 * pc] == hommx::OP_Y)
          return fail(HOMMX_EINVAL, "null points: the criterion reads y (instruction %d), the centroid of the element", pc);
    if (s->threshold != s->threshold) return fail(HOMMX_EINVAL, "the threshold is NaN");
  }
  if (s->reconstruct) {
    if (r.load)
      return fail(HOMMX_EINVAL, "reconstruct together with a load: the reconstruction statistics have no load term (ask for the criterion's "
                                "total_strain / total_flux)");
    if (!s->stats) return fail(HOMMX_EINVAL, "null stats");
    if (int rc = regions_check(src, s->n_regions, s->region, s->region_stats)) return rc;
  }
  return HOMMX_OK;
}

// the argument checks of every entry, in this order: the source, the entry's struct, of a tangent entry the iteration's struct behind
// it, the history, the iteration, the load, the tangent's own or the state's; then a route that forms correctors and, with a load, a
// load solve
int secant_open(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const SecantRequest& r, bool device) {
  auto checks = [&] {
    if (!r.secant) return fail(HOMMX_EINVAL, "null secant arguments");  // a tangent entry's; a null `given` is source_open's
    if (int rc = secant_checks(p, r)) return rc;
    if (r.load || (r.need & NEED_LOAD))
      if (int rc = secant_load_checks(p, r.load)) return rc;
    if (r.tangent)
      if (int rc = secant_tangent_checks(p, r.tangent)) return rc;
    return r.state || (r.need & NEED_STATE) ? secant_state_checks(p, src, r) : HOMMX_OK;
  };
  if (int rc = source_open(p, n_cells, src, r.given, device, checks); rc != GO) return rc;
  return r.load ? secant_load_routes(p) : GO;
}

// what a call holds of a load: the program source of its own beside the coefficient's, and the bytes per cell a chunk holds of it
// beside the caller's array -- the second corrector block, the expansion of a program, the eigenstress
struct SecantLoadPlan {
  bool program = false;
  ProgramLoad prog{};
  size_t scratch = 0;
};
SecantLoadPlan secant_load_plan(const hommx_plan* p, const hommx_secant_load_args* load, hommx_secant_load_args* l) {
  SecantLoadPlan q;
  if (!load) return q;
  const int64_t field = p->n_el * p->ks.t;
  q.program = load_form(load->per_cell) == HOMMX_LOADS_PROGRAM;
  *l = *load;
  if (q.program) {
    l->P = nullptr;
    const hommx_coef_source& s = *load->P_source;
    q.prog = {program_source(s.program, s.n_q, s.table, s.weights, s.params, s.n_fields), &l->P};
  }
  q.scratch = sizeof(double) * (plan_ndof(p) * p->ks.t + (q.program ? field : 0) + (load_eigenstrain(load->per_cell) ? field : 0));
  return q;
}

// The chunk loop of a request that has passed secant_open.  Scratch of a chunk: the current and the candidate stream, the info of its
// eliminations, the slot of a field that does not fit LDS beside the stack (where the chunk rule of the reconstruction does not count
// one already), the tangent stream the caller does not take, and what secant_load_plan counts of a load -- with one the rule is
// load_chunk, since every round ends in a load solve.  Per-cell arrays of the chunk: coef_start / coef_out, history_in / history_out,
// the load array (a program: its expansion, ProgramLoad), the rows of the state's criterion and every output; an absent part's arrays
// are null and take no room.  The labels of a host call travel once, into B_REGION
int secant_call(hommx_plan* p, int64_t n_cells, const hommx_coef_source& s, const double* M, const SecantRequest& r, bool device,
                hipStream_t st) {
  const int64_t t = p->ks.t, field = p->n_el * t, stream = p->n_el * p->ks.n_comp, tan = tangent_stream_doubles(p);
  Chunk<SecantCall> v{};
  hommx_secant_args& a = v.a.s = *r.secant;
  hommx_history_args& h = v.a.h;
  hommx_secant_state_args& ta = v.a.t;
  hommx_secant_tangent_args& g = v.a.g;
  if (r.hist) h = *r.hist;
  if (r.tangent) v.a.has_tangent = true, g = *r.tangent;
  if (r.state) {  // what the checks have passed: members that belong to the half not asked for are not read
    v.a.has_state = true;
    ta = *r.state;
    if (!ta.crit_program) ta.crit_rows = nullptr, ta.crit = ta.crit_values = ta.total_strain = ta.total_flux = nullptr, ta.crit_n_fields = 0;
    if (!ta.reconstruct) ta.n_regions = 0, ta.region = nullptr, ta.stats = ta.region_stats = nullptr;
    if (ta.n_regions && !ta.region) ta.region = s.mask;  // n_regions == 2 of a two-phase source: the mask may be the labels
    if (ta.n_regions && !device) {
      if (int rc = grow(p->buf[B_REGION], p->n_el)) return rc;
      HIP_TRY(hipMemcpy(p->buf[B_REGION].p, ta.region, p->n_el, hipMemcpyHostToDevice));
      ta.region = static_cast<const uint8_t*>(p->buf[B_REGION].p);
    }
  }
  v.a.has_load = r.load != nullptr;
  SecantLoadPlan lp = secant_load_plan(p, r.load, &v.a.l);
  const bool own_slot = secant_slot_used(p, v.a) && recon_in_lds(p);
  const size_t scratch = sizeof(double) * (2 * stream + (own_slot ? plan_ndof(p) : 0) + (v.a.has_tangent && !g.tangent_coef ? tan : 0)) +
                         sizeof(int32_t) + lp.scratch;
  const CellArray in[] = {{&a.rows, hommx::program_row_doubles(a.n_fields)},
                          {&a.xi, t},
                          {&a.coef_start, stream},
                          {&h.history_in, p->n_el * h.n_history},
                          {&v.a.l.P, r.load ? field : 0},
                          {&ta.crit_rows, hommx::program_row_doubles(ta.crit_n_fields)},
                          {&a.points, p->n_el * p->desc.dim, SHARED}};
  const CellArray out[] = {{&a.state, HOMMX_SECANT_NSTATE},
                           {&a.A_eff, t * t, KEPT},
                           {&a.mean_flux, t},
                           {&a.coef_out, stream},
                           {&a.strain, field},
                           {&a.flux, field},
                           {&a.law_values, stream},
                           {&g.tangent, t * t},
                           {&g.asymmetry, 1},
                           {&g.tangent_coef, tan},
                           {&g.tangent_info, 1, PER_CELL, sizeof(int32_t)},
                           {&h.history_out, p->n_el * h.n_history},
                           {&ta.crit, HOMMX_CRIT_NSTATS},
                           {&ta.crit_values, p->n_el},
                           {&ta.total_strain, field},
                           {&ta.total_flux, field},
                           {&ta.stats, HOMMX_RECON_NSTATS(t)},
                           {&ta.region_stats, ta.n_regions * HOMMX_RECON_NREGION(t)}};
  return derived_call(p, n_cells, s, M, v, in, out, &a.info, scratch, r.load ? load_chunk : recon_chunk, device, st,
                      [&](int64_t nc, int64_t chunk, const Chunk<SecantCall>& c) { return secant_run(p, nc, chunk, c, device, st); },
                      nullptr, false, lp.program ? &lp.prog : nullptr);
}

// what every entry of the family is: open the request, then run it
int secant_entry(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* M, const SecantRequest& r, bool device,
                 void* stream = nullptr) {
  if (int rc = secant_open(p, n_cells, src, r, device); rc != GO) return rc;
  return secant_call(p, n_cells, source_of_form(*src), M, r, device, reinterpret_cast<hipStream_t>(stream));
}


// -- second derivatives (hommx_second_sensitivity_source[_device]) ------------------------------------------------------------------------
// bytes per cell of a chunk beside the canonical correctors: the second corrector block and the loads of one direction
size_t sens2_extra(const hommx_plan* p) { return sizeof(double) * p->ks.t * (plan_ndof(p) + p->n_el * p->ks.t); }

// one chunk of at most recon_chunk() cells on the device: the canonical correctors into the plan's scratch, k_sens for the first
// derivatives; then per direction b its loads (k_sens2_loads), their correctors behind the canonical ones (load_correctors), and k_sens2 for the blocks (a, b) and (b, a), a <= b
int sens2_run(hommx_plan* p, int64_t nc, int64_t chunk, const Chunk<hommx_sens2_args>& v, hipStream_t st) {
  const hommx_sens2_args& a = v.a;
  const int t = p->ks.t;
  double *d_A_eff = a.A_eff, *corr = nullptr;
  if (int rc = chunk_correctors(p, nc, chunk, v.coef, v.M, &d_A_eff, a.info, t, st, &corr)) return rc;
  if (a.dA)
    HIP_TRY(hommx::launch_sensitivity(sens_dirs_args(p, corr, v.M, a.n_dirs, a.per_cell, a.dirs, a.dA), nc, st));
  if (int rc = grow(p->buf[B_SENS2], sizeof(double) * chunk * t * p->n_el * t)) return rc;
  hommx::Sens2Args k;
  set_geometry(p, k);
  double* corr_b = corr + chunk * t * k.ndof;
  k.corr = corr;
  k.corr_b = corr_b;
  k.M = v.M;
  k.n_dirs = a.n_dirs;
  k.per_cell = a.per_cell != 0;
  k.dirs = a.dirs;
  k.P = static_cast<double*>(p->buf[B_SENS2].p);
  k.d2A = a.d2A;
  for (int b = 0; b < a.n_dirs; ++b) {
    k.b = b;
    HIP_TRY(hommx::launch_sens2_loads(k, nc, st));
    if (int rc = load_correctors(p, nc, chunk, v.coef, v.M, hommx::LoadOverride{k.P, t, true}, st, corr_b)) return rc;  // t per-cell loads
    HIP_TRY(hommx::launch_sens2(k, nc, st));
  }
  if (v.curv) {
    // the curvature term: dA_H along the second-order streams of the chunk, every pair a <= b in one launch of k_sens (it loops over its
    // directions at run time; HOMMX_SENS_MAX_DIRS bounds the ABI, not the kernel), behind the streams; then d2A[a][b] += dA_H[pair(a, b)]
    const int n_pairs = tangent_pairs(a.n_dirs);
    double* dAk = v.curv + chunk * n_pairs * p->n_el * p->ks.n_comp;
    HIP_TRY(hommx::launch_sensitivity(sens_dirs_args(p, corr, v.M, n_pairs, 1, v.curv, dAk), nc, st));
    HIP_TRY(hommx::launch_sens2_add_curvature(a.d2A, dAk, a.n_dirs, t, nc, st));
  }
  return HOMMX_OK;
}

// the argument checks of both entry points -- the frontal mesh route among them: the descriptor of a mesh plan names its route --, then
// the routes the call needs: one that forms correctors and a load solve
int sens2_open(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const hommx_sens2_args* a, bool device) {
  auto checks = [&] {
    if (a->n_dirs < 1 || a->n_dirs > HOMMX_SENS_MAX_DIRS)
      return fail(HOMMX_EINVAL, "n_dirs must be 1 .. %d, got %d", HOMMX_SENS_MAX_DIRS, a->n_dirs);
    if (parameter_dirs(a->per_cell))
      if (int rc = parameter_dirs_check(src, a->n_dirs, a->dirs)) return rc;
    if ((!a->dirs && !parameter_dirs(a->per_cell)) || !a->d2A) return fail(HOMMX_EINVAL, "null dirs / d2A");
    if (p->desc.n_micro == 0 && !(p->desc.flags & (HOMMX_MESH_FLAG_TREE | HOMMX_MESH_FLAG_LOADS)))
      return fail(HOMMX_EINVAL, "the frontal mesh route (mesh_front) solves for the canonical loads only: second derivatives need the load "
                                "solve of a plan of the tree route (HOMMX_MESH_FLAG_TREE, route=\"tree\")");
    return HOMMX_OK;
  };
  if (int rc = source_open(p, n_cells, src, a, device, checks); rc != GO) return rc;
  if (int rc = load_workspace(p)) return rc;
  return GO;
}

int sens2_call(hommx_plan* p, int64_t n_cells, const hommx_coef_source& s, const double* M, const hommx_sens2_args& args, bool device,
               hipStream_t st) {
  const int64_t tt = p->ks.t * p->ks.t, el = p->n_el * p->ks.n_comp;
  Chunk<hommx_sens2_args> v{};
  hommx_sens2_args& a = v.a = args;
  const CellArray in[] = {{&a.dirs, a.n_dirs * el, a.per_cell ? PER_CELL : SHARED}};
  const CellArray out[] = {{&a.d2A, a.n_dirs * a.n_dirs * tt}, {&a.A_eff, tt, KEPT}, {&a.dA, a.n_dirs * tt}};
  return derived_call(p, n_cells, s, M, v, in, out, &a.info, sens2_extra(p), load_chunk, device, st,
                      [&](int64_t nc, int64_t chunk, const Chunk<hommx_sens2_args>& c) { return sens2_run(p, nc, chunk, c, st); },
                      parameter_dirs(a.per_cell) ? &a.dirs : nullptr, curvature_dirs(a.per_cell));
}

}  // namespace

extern "C" {

int hommx_reconstruct_batch_device(hommx_plan* p, int64_t n_cells, const double* d_coef, const double* d_M, const double* d_xi, double* d_stats,
                                   double* d_strain, double* d_flux, double* d_A_eff, int32_t* d_info, void* stream) {
  const ReconCall a{d_xi, 0, nullptr, d_stats, nullptr, d_strain, d_flux, d_A_eff, d_info};
  if (int rc = recon_open(p, n_cells, d_coef, a, true, [] { return HOMMX_OK; }); rc != GO) return rc;
  return recon_call(p, n_cells, sampled_source(d_coef), d_M, a, true, reinterpret_cast<hipStream_t>(stream));
}

int hommx_reconstruct_batch(hommx_plan* p, int64_t n_cells, const double* coef, const double* M, const double* xi, double* stats, double* strain,
                            double* flux, double* A_eff, int32_t* info) {
  const ReconCall a{xi, 0, nullptr, stats, nullptr, strain, flux, A_eff, info};
  if (int rc = recon_open(p, n_cells, coef, a, false, [] { return HOMMX_OK; }); rc != GO) return rc;
  return recon_call(p, n_cells, sampled_source(coef), M, a, false, nullptr);
}

int hommx_reconstruct_source_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* d_M, const double* d_xi,
                                    int32_t n_regions, const uint8_t* d_region, double* d_stats, double* d_region_stats, double* d_strain,
                                    double* d_flux, double* d_A_eff, int32_t* d_info, void* stream) {
  const ReconCall a{d_xi, n_regions, d_region, d_stats, d_region_stats, d_strain, d_flux, d_A_eff, d_info};
  auto more = [&] {
    if (int rc = coef_check(p, src)) return rc;
    return regions_check(src, n_regions, d_region, d_region_stats);
  };
  if (int rc = recon_open(p, n_cells, src, a, true, more); rc != GO) return rc;
  return recon_call(p, n_cells, source_of_form(*src), d_M, a, true, reinterpret_cast<hipStream_t>(stream));
}

int hommx_reconstruct_source(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* M, const double* xi, int32_t n_regions,
                             const uint8_t* region, double* stats, double* region_stats, double* strain, double* flux, double* A_eff,
                             int32_t* info) {
  const ReconCall a{xi, n_regions, region, stats, region_stats, strain, flux, A_eff, info};
  auto more = [&] {
    if (int rc = coef_check(p, src)) return rc;
    return regions_check(src, n_regions, region, region_stats);
  };
  if (int rc = recon_open(p, n_cells, src, a, false, more); rc != GO) return rc;
  return recon_call(p, n_cells, source_of_form(*src), M, a, false, nullptr);
}

int hommx_sensitivity_source_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* d_M, const hommx_sens_args* args,
                                    void* stream) {
  if (int rc = source_open(p, n_cells, src, args, true, [&] { return sens_checks(src, args); }); rc != GO) return rc;
  return sens_call(p, n_cells, source_of_form(*src), d_M, *args, true, reinterpret_cast<hipStream_t>(stream));
}

int hommx_sensitivity_source(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* M, const hommx_sens_args* args) {
  if (int rc = source_open(p, n_cells, src, args, false, [&] { return sens_checks(src, args); }); rc != GO) return rc;
  return sens_call(p, n_cells, source_of_form(*src), M, *args, false, nullptr);
}

int hommx_stratification_sensitivity_source_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                                   const hommx_strat_sens_args* args, void* stream) {
  if (int rc = source_open(p, n_cells, src, args, true, [&] { return strat_checks(args); }); rc != GO) return rc;
  return strat_call(p, n_cells, source_of_form(*src), d_M, *args, true, reinterpret_cast<hipStream_t>(stream));
}

int hommx_stratification_sensitivity_source(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* M,
                                            const hommx_strat_sens_args* args) {
  if (int rc = source_open(p, n_cells, src, args, false, [&] { return strat_checks(args); }); rc != GO) return rc;
  return strat_call(p, n_cells, source_of_form(*src), M, *args, false, nullptr);
}

int hommx_loads_source_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* d_M, const hommx_load_args* args,
                               void* stream) {
  if (int rc = loads_open(p, n_cells, src, args, true); rc != GO) return rc;
  return loads_call(p, n_cells, source_of_form(*src), d_M, *args, true, reinterpret_cast<hipStream_t>(stream));
}

int hommx_loads_source(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* M, const hommx_load_args* args) {
  if (int rc = loads_open(p, n_cells, src, args, false); rc != GO) return rc;
  return loads_call(p, n_cells, source_of_form(*src), M, *args, false, nullptr);
}

int hommx_criterion_source_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                  const hommx_criterion_args* args, void* stream) {
  if (int rc = crit_open(p, n_cells, src, args, true); rc != GO) return rc;
  return crit_call(p, n_cells, source_of_form(*src), d_M, *args, true, reinterpret_cast<hipStream_t>(stream));
}

int hommx_criterion_source(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* M, const hommx_criterion_args* args) {
  if (int rc = crit_open(p, n_cells, src, args, false); rc != GO) return rc;
  return crit_call(p, n_cells, source_of_form(*src), M, *args, false, nullptr);
}

int hommx_secant_source_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* d_M, const hommx_secant_args* args,
                               void* stream) {
  return secant_entry(p, n_cells, src, d_M, secant_request(args), true, stream);
}

int hommx_secant_source(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* M, const hommx_secant_args* args) {
  return secant_entry(p, n_cells, src, M, secant_request(args), false);
}

int hommx_secant_tangent_source_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                       const hommx_secant_tangent_args* args, void* stream) {
  return secant_entry(p, n_cells, src, d_M, secant_request(args), true, stream);
}

int hommx_secant_tangent_source(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* M,
                                const hommx_secant_tangent_args* args) {
  return secant_entry(p, n_cells, src, M, secant_request(args), false);
}

int hommx_secant_history_source_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                       const hommx_secant_args* args, const hommx_history_args* history, void* stream) {
  return secant_entry(p, n_cells, src, d_M, secant_request(args, NEED_HISTORY, history), true, stream);
}

int hommx_secant_history_source(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* M, const hommx_secant_args* args,
                                const hommx_history_args* history) {
  return secant_entry(p, n_cells, src, M, secant_request(args, NEED_HISTORY, history), false);
}

int hommx_secant_tangent_history_source_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                               const hommx_secant_tangent_args* args, const hommx_history_args* history, void* stream) {
  return secant_entry(p, n_cells, src, d_M, secant_request(args, NEED_HISTORY, history), true, stream);
}

int hommx_secant_tangent_history_source(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* M,
                                        const hommx_secant_tangent_args* args, const hommx_history_args* history) {
  return secant_entry(p, n_cells, src, M, secant_request(args, NEED_HISTORY, history), false);
}

int hommx_secant_load_source_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                    const hommx_secant_args* args, const hommx_history_args* history, const hommx_secant_load_args* load,
                                    void* stream) {
  return secant_entry(p, n_cells, src, d_M, secant_request(args, NEED_LOAD, history, load), true, stream);
}

int hommx_secant_load_source(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* M, const hommx_secant_args* args,
                             const hommx_history_args* history, const hommx_secant_load_args* load) {
  return secant_entry(p, n_cells, src, M, secant_request(args, NEED_LOAD, history, load), false);
}

int hommx_secant_state_source_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                     const hommx_secant_args* args, const hommx_history_args* history, const hommx_secant_load_args* load,
                                     const hommx_secant_state_args* state, void* stream) {
  return secant_entry(p, n_cells, src, d_M, secant_request(args, NEED_STATE, history, load, state), true, stream);
}

int hommx_secant_state_source(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* M, const hommx_secant_args* args,
                              const hommx_history_args* history, const hommx_secant_load_args* load, const hommx_secant_state_args* state) {
  return secant_entry(p, n_cells, src, M, secant_request(args, NEED_STATE, history, load, state), false);
}

int hommx_secant_tangent_load_source_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                            const hommx_secant_tangent_args* args, const hommx_history_args* history,
                                            const hommx_secant_load_args* load, void* stream) {
  return secant_entry(p, n_cells, src, d_M, secant_request(args, NEED_LOAD, history, load), true, stream);
}

int hommx_secant_tangent_load_source(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* M,
                                     const hommx_secant_tangent_args* args, const hommx_history_args* history,
                                     const hommx_secant_load_args* load) {
  return secant_entry(p, n_cells, src, M, secant_request(args, NEED_LOAD, history, load), false);
}


int hommx_second_sensitivity_source_device(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                           const hommx_sens2_args* args, void* stream) {
  if (int rc = sens2_open(p, n_cells, src, args, true); rc != GO) return rc;
  return sens2_call(p, n_cells, source_of_form(*src), d_M, *args, true, reinterpret_cast<hipStream_t>(stream));
}

int hommx_second_sensitivity_source(hommx_plan* p, int64_t n_cells, const hommx_coef_source* src, const double* M, const hommx_sens2_args* args) {
  if (int rc = sens2_open(p, n_cells, src, args, false); rc != GO) return rc;
  return sens2_call(p, n_cells, source_of_form(*src), M, *args, false, nullptr);
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
