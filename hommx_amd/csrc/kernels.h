// kernels.h -- internal launch interface between the C ABI (api.hip) and the kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/hommx_hip.h"
#include "coef_program.h"

namespace hommx {

// unknowns per node, tensor size and coefficient components per element of a problem kind (include/hommx_hip.h)
struct KindSizes {
  int bs, t, n_comp;
};
constexpr KindSizes kind_sizes(int dim, int kind) {
  const int te = dim * (dim + 1) / 2;  // elasticity (Voigt) tensor size
  return kind == HOMMX_KIND_POISSON_SCALAR   ? KindSizes{1, dim, 1}
         : kind == HOMMX_KIND_POISSON_MATRIX ? KindSizes{1, dim, te}
         : kind == HOMMX_KIND_ELASTICITY_ISO ? KindSizes{dim, te, 2}
                                             : KindSizes{dim, te, te * (te + 1) / 2};
}

// f(DIM, KIND) with the (validated) dim in {2, 3} and kind in 0..3 of a plan as std::integral_constants: the one list of the eight
// (DIM, KIND) pairs the kernels are instantiated for
template <typename F>
auto dispatch_dim_kind(int dim, int kind, F&& f) {
  auto with_dim = [&](auto D) {
    switch (kind) {
      case 0: return f(D, std::integral_constant<int, 0>{});
      case 1: return f(D, std::integral_constant<int, 1>{});
      case 2: return f(D, std::integral_constant<int, 2>{});
      default: return f(D, std::integral_constant<int, 3>{});
    }
  };
  return dim == 2 ? with_dim(std::integral_constant<int, 2>{}) : with_dim(std::integral_constant<int, 3>{});
}

// Where the per-element coefficient of a scalar Poisson cell comes from (device samplers).
//   STREAM      coef[cell][n_el]: element means sampled by the caller
//   TWO_PHASE   mask[n_el] (uint8) selects coef[cell][0 / 1]
//   AFFINE      A_K = a + b * table[K]                      coef[cell] = (a, b); table[n_el] = element means of g(y)
//   RECIPROCAL  A_K = sum_q w[q] / (a + b * table[K][q])    coef[cell] = (a, b); table[n_el][nq] = g at the quadrature points
// Every operation of AFFINE / RECIPROCAL is a separately rounded IEEE operation in a fixed order, so a host that evaluates the
// same formula (hommx_amd.hmm.Separable.host_stream) gets the same bits.
// separately rounded IEEE operations: hipcc contracts a * b + c into an fma by default (and __dmul_rn / __dadd_rn are plain
// operators in the HIP headers), which a host evaluating the same formula with NumPy does not do
__device__ __forceinline__ double mul_rn(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ double add_rn(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ double div_rn(double a, double b) {
#pragma clang fp contract(off)
  return a / b;
}
enum CoefMode { COEF_STREAM = 0, COEF_TWO_PHASE = 1, COEF_AFFINE = 2, COEF_RECIPROCAL = 3 };
struct CoefSource {
  int mode = COEF_STREAM;
  int nq = 0;
  const void* table = nullptr;    // mask (uint8) or table (double)
  const double* weights = nullptr;
};

// fused2d.hip: 2D scalar Poisson (optionally stratified), 3 <= n <= 32, one wave per macro cell.
hipError_t launch_poisson2d_fused(const double* d_coef, const double* d_M, double* d_out, int32_t* d_info,
                                  int n, long long ncells, hipStream_t stream, CoefSource src = CoefSource());
// fused2d_iso.hip: the same for unstratified cells (no M): launch_poisson2d_fused hands every call with d_M == nullptr to it
hipError_t launch_poisson2d_fused_iso(const double* d_coef, double* d_out, int32_t* d_info, int n, long long ncells, hipStream_t stream,
                                      CoefSource src);

// The factor record of one cell, written by k_poisson2d_fused<NB, true> and read by k_fused2d_subst<NB> and k_fused2d_subst_rhs<NB> (NB = 16 for
// n <= 16, else 32); private to the three kernels.  In doubles, with N' = -S^-1 as the elimination carries it:
//   header  [C e0 (NB) | C e1 (NB) | y_last (2 NB) | M (4) | esh (1) | pad (3)]   C = the wrap coupling E_{n-1}, y_last = z of the final sweep,
//                                                                                esh = the magnitude exponent of the cell
//   step j  [N'_j (NB NB, register-major [ti][tj][r][lane]) | N'_j r~_j (2 NB) | E_j e0 (NB) | E_j e1 (NB)],  j = 0 .. n-2
//   last    [N'_last (NB NB, register-major)]                                     the inverse of the gauged last Schur block, behind step n-2
// e0[i] = E[i][i], e1[i] = E[i][i-1] (cyclic on the real indices, padding first).  n = NB = 32: 136 + 31 * 1152 + 1024 = 36,872 doubles =
// 294,976 bytes per cell; n = NB = 16: 72 + 15 * 320 + 256 = 5,128 doubles = 41,024 bytes.  k_fused2d_subst reads neither esh nor the last block.
constexpr long long fused_fact_header(int NB) { return 4 * NB + 8; }
constexpr long long fused_fact_step(int NB) { return (long long)NB * NB + 4 * NB; }
constexpr long long fused_fact_doubles(int n) {
  return fused_fact_header(n <= 16 ? 16 : 32) + (n - 1) * fused_fact_step(n <= 16 ? 16 : 32) + (n <= 16 ? 16 * 16 : 32 * 32);
}
// fused2d.hip: the same elimination of an element stream, and the factor record of every cell into d_fact[ncells][fused_fact_doubles(n)]
hipError_t launch_poisson2d_fused_fact(const double* d_coef, const double* d_M, double* d_out, int32_t* d_info, int n, long long ncells,
                                       hipStream_t stream, double* d_fact);
// fused2d_subst.hip: correctors d_corr[ncells][2][n n] (dof = i + n j, mean-free) by substitution on the factor records, one wave per cell
hipError_t launch_fused2d_subst(const double* d_fact, double* d_corr, int n, long long ncells, hipStream_t stream);
// fused2d_rhs.hip: the correctors of user loads by substitution on the same records: rows l < n_loads of d_corr[ncells][2][n n] (mean-free; the
// other rows are not written) solve K chi_l = -f^l with f^l of P[n_loads][2 n n][2] (per_cell: P[ncells][n_loads][2 n n][2]) as loads.hip
// forms it; d_M [ncells][2][2] or null
hipError_t launch_fused2d_subst_rhs(const double* d_fact, const double* d_P, int n_loads, bool per_cell, const double* d_M, double* d_corr, int n,
                                    long long ncells, hipStream_t stream);
// one step of iterative refinement of the canonical correctors of a fused 2D plan on its own record: the residual is the load vector of the
// canonical flux field, the correction its load corrector (fused2d_rhs.hip).  Scratch: d_q 8 n^2 doubles, d_delta 2 n^2 doubles per cell
hipError_t launch_fused2d_refine(const double* d_fact, const double* d_coef, const double* d_M, double* d_corr, double* d_q, double* d_delta, int n,
                                 long long ncells, hipStream_t stream);

// assembly.hip: coef[cell][el][comp] of a separable coefficient (AFFINE / RECIPROCAL; params[cell][comp] = (a, b)) expanded into the element stream
hipError_t launch_expand_separable(CoefSource src, const double* d_params, double* d_coef, long long n_el, int n_comp, long long ncells,
                                   hipStream_t stream);

// assembly.hip: coef[cell][el][comp] = mask[el] ? values[cell][1][comp] : values[cell][0][comp]
hipError_t launch_expand_two_phase(const unsigned char* d_mask, const double* d_values, double* d_coef, long long n_el,
                                   int n_comp, long long ncells, hipStream_t stream);

// What every kernel that walks the elements of a cell with one workgroup per macro cell reads (elem_walk.h): the element geometry, the
// correctors, M and the (dim, kind, mesh) its launcher dispatches on.  The base of the argument structs below; api.hip::set_geometry
// fills everything but corr and M from the plan
struct ElemWalk {
  int dim = 0, kind = 0;             // of the plan
  bool mesh = false;                 // a mesh plan: the geometry is read; else computed in the kernel
  int n = 0;                         // structured plans: micro cells per side
  double vol_struct = 0.0;           // structured plans: element volume
  long long ndof = 0, n_el = 0;      // periodic unknowns (nodes x bs) and elements per cell
  const int32_t* el_nodes = nullptr; // mesh plans: [n_el][dim+1] periodic nodes, [n_el][dim+1][dim] P1 gradients, [n_el] volumes
  const double* grads = nullptr;
  const double* vol = nullptr;
  const double* corr = nullptr;      // [nc][t][ndof]
  const double* M = nullptr;         // [nc][d][d] or null
};

// reconstruct.hip: per-element gradient / strain and flux / stress of `nc` cells from their correctors, and the per-cell statistics
// [mean_strain (t) | mean_flux (t) | energy | max_flux | argmax_element] (include/hommx_hip.h, hommx_reconstruct_batch)
struct ReconArgs : ElemWalk {
  const double* coef = nullptr;      // [nc][n_el][n_comp]
  const double* xi = nullptr;        // [nc][t]
  double* stats = nullptr;           // [nc][2t+3]
  double* strain = nullptr;          // [nc][n_el][t] or null (then flux is null as well: no fields)
  double* flux = nullptr;
  double* slot = nullptr;            // [nc][ndof] scratch for chi^xi of cells too large for LDS (null: LDS)
  // per-region statistics (hommx_reconstruct_source): n_regions > 0 selects the REGIONS instantiations
  int n_regions = 0;
  const uint8_t* region = nullptr;   // [n_el] label of every element; >= n_regions: in no region
  double* region_stats = nullptr;    // [nc][n_regions][2t+4] = [volume | the 2t+3 statistics over the region]
};
// bytes of chi^xi above which a cell takes a scratch slot instead of LDS
size_t recon_lds_limit();
hipError_t launch_reconstruct(const ReconArgs& a, long long nc, hipStream_t stream);

// sensitivity.hip: derivatives of A_H along coefficient directions and its per-element gradient, from the correctors of `nc` cells
// (include/hommx_hip.h, hommx_sensitivity_source)
struct SensArgs : ElemWalk {
  int n_dirs = 0;                    // 0 .. HOMMX_SENS_MAX_DIRS
  bool per_cell = false;             // dirs[nc][n_dirs][n_el][n_comp] instead of dirs[n_dirs][n_el][n_comp]
  const double* dirs = nullptr;
  double* dA = nullptr;              // [nc][n_dirs][t][t]
  const double* weights = nullptr;   // [nc][t][t], with grad[nc][n_el][n_comp]; or both null
  double* grad = nullptr;
};
hipError_t launch_sensitivity(const SensArgs& a, long long nc, hipStream_t stream);

// sens2.hip: second derivatives of A_H along coefficient directions (include/hommx_hip.h, hommx_second_sensitivity_source; DESIGN.md
// section 4.13), one direction b per launch.  launch_sens2_loads: the polarisation loads P^{b,m} = material(dir_b) s^m from the canonical
// correctors (corr); launch_sens2: d2A[a][b] and d2A[b][a], a <= b, from the canonical correctors and the correctors of those loads
struct Sens2Args : ElemWalk {
  const double* corr_b = nullptr;    // [nc][t][ndof]: the correctors of the loads of direction b (k_sens2)
  int n_dirs = 0;                    // 1 .. HOMMX_SENS_MAX_DIRS
  int b = 0;                         // the direction of this launch
  bool per_cell = false;             // dirs[nc][n_dirs][n_el][n_comp] instead of dirs[n_dirs][n_el][n_comp]
  const double* dirs = nullptr;
  double* P = nullptr;               // [nc][t][n_el][t]: written by k_sens2_loads, a per-cell load block of loads.hip
  double* d2A = nullptr;             // [nc][n_dirs][n_dirs][t][t] (k_sens2)
};
hipError_t launch_sens2_loads(const Sens2Args& a, long long nc, hipStream_t stream);
hipError_t launch_sens2(const Sens2Args& a, long long nc, hipStream_t stream);
// the curvature term of HOMMX_DIRS_PARAMETERS_CURVATURE: d2A[nc][n_dirs][n_dirs][t][t] += dAk[nc][n_pairs][t][t], the first derivatives
// along the second-order streams of the pairs a <= b in row-major order, one separately rounded addition per entry
hipError_t launch_sens2_add_curvature(double* d2A, const double* dAk, int n_dirs, int t, long long nc, hipStream_t stream);

// sens_strat.hip: derivatives of A_H with respect to the stratification M and their product with caller weights, from the correctors
// of `nc` cells (include/hommx_hip.h, hommx_stratification_sensitivity_source)
struct StratSensArgs : ElemWalk {
  const double* coef = nullptr;      // [nc][n_el][n_comp]
  double* dA_dM = nullptr;           // [nc][d][d][t][t] or null
  const double* weights = nullptr;   // [nc][t][t], with grad_M[nc][d][d]; or both null
  double* grad_M = nullptr;
};
hipError_t launch_sens_strat(const StratSensArgs& a, long long nc, hipStream_t stream);

// loads.hip: user-supplied polarisation loads P[load][el][t] (include/hommx_hip.h, hommx_loads_source).
// launch_polar: P_eff from the canonical correctors in corr (Levin); launch_load_stats: the response outputs from the correctors of the
// loads themselves in corr (rows >= n_loads unused), every one of them optional
struct LoadArgs : ElemWalk {
  const double* coef = nullptr;      // [nc][n_el][n_comp] (k_load_stats)
  int n_loads = 0;                   // 1 .. t
  bool per_cell = false;             // P[nc][n_loads][n_el][t] instead of P[n_loads][n_el][t]
  const double* P = nullptr;
  double* P_eff = nullptr;           // [nc][n_loads][t] (k_polar)
  double* energy = nullptr;          // [nc][n_loads][n_loads] or null
  double* stats = nullptr;           // [nc][n_loads][t+2] or null
  double* strain = nullptr;          // [nc][n_loads][n_el][t] or null (then flux is null as well)
  double* flux = nullptr;
};
hipError_t launch_polar(const LoadArgs& a, long long nc, hipStream_t stream);
hipError_t launch_load_stats(const LoadArgs& a, long long nc, hipStream_t stream);
// k_eigenstress: P[nc][n_loads][n_el][t] = -(material(coef[nc][n_el][n_comp]) E), E[nc][n_loads][n_el][t] (per_cell) or [n_loads][n_el][t]
// in the components of the reconstruction's strain (shear doubled); P may be E itself when per_cell
hipError_t launch_eigenstress(int dim, int kind, const double* coef, const double* E, bool per_cell, double* P, int n_loads, long long n_el,
                              long long nc, hipStream_t stream);

// criterion.hip: a failure criterion -- one scalar program of the element's strain, flux and coefficient -- on the reconstructed micro
// state of `nc` cells, and its per-cell statistics (include/hommx_hip.h, hommx_criterion_source)
struct CritArgs : ElemWalk {
  const double* coef = nullptr;      // [nc][n_el][n_comp]
  const double* xi = nullptr;        // [nc][t]
  ProgramArgs prog;                  // n_comp == 1; `X k` reads the row [midpoint (3) | fields | strain (t) | flux (t) | coefficient (n_comp)]
  int n_fields = 0;
  const double* rows = nullptr;      // [nc][3 + n_fields]
  const double* points = nullptr;    // [n_el][dim] element centroids, or null (no Y in the program)
  double threshold = 1.0;
  const double* corr_load = nullptr; // [nc][t][ndof]: row 0 is the corrector of the load, or null (no load: P is null as well)
  const double* P = nullptr;         // [n_el][t] or, per_cell, [nc][n_el][t]
  bool per_cell = false;
  double* crit = nullptr;            // [nc][4] = [max | argmax element | sum |K| v | sum |K| [v >= threshold]]
  double* values = nullptr;          // [nc][n_el] or null
  double* strain = nullptr;          // [nc][n_el][t] or null (then flux is null as well)
  double* flux = nullptr;
  double* slot = nullptr;            // [nc][ndof] scratch for the field of cells that do not fit LDS beside the stack (null: LDS)
};
// dynamic LDS of k_criterion with the field in it: the field and the stack rows below the top, one of kWalkThreads doubles per level
size_t criterion_lds_bytes(long long ndof, int depth);
// depth: the maximal stack depth of the (validated) program
hipError_t launch_criterion(const CritArgs& a, int depth, long long nc, hipStream_t stream);

// criterion_state.hip: a criterion of the NONLINEAR state behind the last round of a secant chunk (include/hommx_hip.h,
// hommx_secant_state_source): k_criterion on the stopped stream (coef: `cur`), whose program may also read the
// base coefficient and the history at the start of the call
struct CritStateArgs : CritArgs {
  const double* base = nullptr;      // [nc][n_el][n_comp]: what b[k] reads
  const double* hist_in = nullptr;   // [nc][n_el][n_history]: what h[k] reads, or null (n_history == 0)
  int n_history = 0;                 // 0 .. HOMMX_SECANT_MAX_HISTORY; prog's row is [.. | c (n_comp) | h (n_history) | b (n_comp)]
};
// dynamic LDS as k_criterion's (criterion_lds_bytes); depth: the maximal stack depth of the (validated) program
hipError_t launch_criterion_state(const CritStateArgs& a, int depth, long long nc, hipStream_t stream);

// secant.hip: one round of the secant iteration of a strain-dependent coefficient on `nc` cells (include/hommx_hip.h,
// hommx_secant_source).  A cell whose state says it has stopped is not touched
struct SecantArgs : ElemWalk {
  const double* base = nullptr;      // [nc][n_el][n_comp]: what c[k] reads
  double* cur = nullptr;             // [nc][n_el][n_comp]: the current stream, the one the correctors belong to; receives the candidate
  double* cand = nullptr;            // [nc][n_el][n_comp]: the candidate stream w
  const double* xi = nullptr;        // [nc][t]
  ProgramArgs prog;                  // n_comp == the plan's; the row of k_criterion
  int n_fields = 0;
  const double* rows = nullptr;      // [nc][3 + n_fields]
  const double* points = nullptr;    // [n_el][dim] element centroids, or null (no Y in the program)
  int round = 0, max_iter = 1;       // the round j this launch is, of at most max_iter
  double tol = 0.0, relax = 1.0;
  const int32_t* info = nullptr;     // [nc]: of the elimination of this round
  double* state = nullptr;           // [nc][3] = [rounds | change | status], status -1 while the cell runs
  double* mean_flux = nullptr;       // [nc][t] or null
  double* law_values = nullptr;      // [nc][n_el][n_comp] or null
  double* strain = nullptr;          // [nc][n_el][t] or null (then flux is null as well)
  double* flux = nullptr;
  double* slot = nullptr;            // [nc][ndof] scratch for the field of cells that do not fit LDS beside the stack (null: LDS)
};
// dynamic LDS as k_criterion's (criterion_lds_bytes); depth: the maximal stack depth of the (validated) program
hipError_t launch_secant(const SecantArgs& a, int depth, long long nc, hipStream_t stream);
// the same round for a law with history variables (hommx_secant_history_source): prog stores n_comp + n_history
// values, and its row is longer by the n_history entries h reads
struct SecantHistoryArgs : SecantArgs {
  const double* hist_in = nullptr;   // [nc][n_el][n_history]: what h[k] reads in every round, the history at the start of the call
  double* hist_out = nullptr;        // [nc][n_el][n_history]: the updates of the stopping round; hist_in's bits for status 2 or 3
  int n_history = 0;                 // 1 .. HOMMX_SECANT_MAX_HISTORY
};
hipError_t launch_secant_history(const SecantHistoryArgs& a, int depth, long long nc, hipStream_t stream);

// secant_tangent.hip: the coefficient of the consistent tangent of the secant response on `nc` cells whose iteration has ended
// (include/hommx_hip.h, hommx_secant_tangent_source): T_K = material(cur_K) + sum_k g_k (dL_k/de)^T, its
// symmetric part as an element stream of the tangent kind and the asymmetry of the cell
struct SecantTangentArgs : ElemWalk {
  const double* base = nullptr;      // [nc][n_el][n_comp]: what c[k] reads
  const double* cur = nullptr;       // [nc][n_el][n_comp]: the stream the correctors belong to
  const double* xi = nullptr;        // [nc][t]
  ProgramArgs prog;                  // the law; it reads no s entry
  int n_fields = 0;
  const double* rows = nullptr;      // [nc][3 + n_fields]
  const double* points = nullptr;    // [n_el][dim] element centroids, or null (no Y in the program)
  const double* state = nullptr;     // [nc][3]: the status decides between the tangent (0, 1) and the identity material (2, 3)
  double* tan = nullptr;             // [nc][n_el][t (t + 1) / 2] in the component order of the tangent kind
  double* asym = nullptr;            // [nc]: max |T - T^T| / max |T|, NaN for a cell of status 2 or 3
  double* slot = nullptr;            // [nc][ndof] scratch for the field of cells that do not fit LDS beside the stack (null: LDS)
};
// the kind of the element stream k_secant_tangent writes for a plan of `kind`: the full symmetric t x t coefficient
constexpr int tangent_kind(int kind) { return kind < 2 ? HOMMX_KIND_POISSON_MATRIX : HOMMX_KIND_ELASTICITY_VOIGT; }
// the slots P of one sweep of the forward mode for a program of stack depth `depth` on a plan of tensor size t: t for t <= 3 and 2
// for t = 6 where the stack rows of that width fit recon_lds_limit(), else 1 (which fits at every depth)
int secant_tangent_slots(int t, int depth);
// dynamic LDS of k_secant_tangent<.., P> with the field in it: the field and the stack rows below the top,
// stack[depth - 1][1 + P][kWalkThreads]
size_t secant_tangent_lds_bytes(long long ndof, int depth, int slots);
hipError_t launch_secant_tangent(const SecantTangentArgs& a, int depth, long long nc, hipStream_t stream);
// the same for a law with history variables: prog is the law TRUNCATED behind the last component's STORE (the updates are not
// differentiated, and nothing is written to a history), and h[k] reads hist_in
struct SecantTangentHistoryArgs : SecantTangentArgs {
  const double* hist_in = nullptr;   // [nc][n_el][n_history]
  int n_history = 0;
};
hipError_t launch_secant_tangent_history(const SecantTangentHistoryArgs& a, int depth, long long nc, hipStream_t stream);
// tangent[cell][tt] = NaN for every cell whose status (state[cell][2]) is 2 or 3
hipError_t launch_tangent_mask(const double* state, double* tangent, int tt, long long nc, hipStream_t stream);

// secant_load.hip: the round and the tangent coefficient beside ONE load per cell (include/hommx_hip.h, hommx_secant_load_source;
// DESIGN.md section 4.18).  What a loaded round reads beside SecantArgs:
struct RoundLoad {
  const double* chi = nullptr;       // [nc][t][ndof]: row 0 of a cell is the corrector of its load on the current stream
  const double* P = nullptr;         // [nc][n_el][t]: the polarisation, or null (the eigenstrain code)
  const double* E = nullptr;         // [nc][n_el][t]: the eigenstrain, or null (the polarisation code); exactly one of the two is set
};
// n_history == 0: a law without history variables (hist_in and hist_out are then not read)
struct SecantLoadArgs : SecantHistoryArgs {
  RoundLoad load;
};
hipError_t launch_secant_load(const SecantLoadArgs& a, int depth, long long nc, hipStream_t stream);
// the tangent at the strain the law saw: the total one beside a polarisation (E null), the elastic one beside an eigenstrain
struct SecantTangentLoadArgs : SecantTangentHistoryArgs {
  const double* corr_load = nullptr; // [nc][t][ndof]: row 0 is the corrector of the load on `cur`
  const double* E = nullptr;         // [nc][n_el][t] or null
};
hipError_t launch_secant_tangent_load(const SecantTangentLoadArgs& a, int depth, long long nc, hipStream_t stream);

// the loads a corrector pass of the blocked family solves for instead of the canonical ones: rows l < n_loads of Brhs from P (device), the
// rest zero.  P starts at the first cell of the call
struct LoadOverride {
  const double* P = nullptr;         // [n_loads][n_el][t] or, per_cell, [ncells][n_loads][n_el][t]
  int n_loads = 0;
  bool per_cell = false;
};

// calibrate.hip: best sustained v_mfma_f64_16x16x4_f64 and v_fma_f64 rates over 2 and 4 waves per SIMD.
hipError_t run_fp64_calibration(double* mfma_flops_per_s, double* fma_flops_per_s, double* mfma_lds_fed_flops_per_s = nullptr);

}  // namespace hommx

namespace hommx {
// blocked.hip: the blocked family (any dim / kind / n) as api.hip sees it; everything else of the family is in blocked_internal.h
struct BlockedWorkspace;
int blocked_workspace_create(BlockedWorkspace** out, int dim, int n, int kind);
void blocked_workspace_destroy(BlockedWorkspace* ws);
// `loads` (with d_corr): the correctors of these loads instead of the canonical ones, on the route that forms correctors; d_out then
// holds C0 - f^T K^+ f, which is no effective tensor
int blocked_solve(BlockedWorkspace* ws, long long ncells, const double* d_coef, const double* d_M,
                  double* d_out, int32_t* d_info, hipStream_t stream, double* d_corr = nullptr, const LoadOverride* loads = nullptr);
// allocate the workspace of the route for batches of up to n_cells (what the first solve would otherwise do)
int blocked_reserve(BlockedWorkspace* ws, long long n_cells);
// "small_wave" (b <= 48), "small_fused" (48 < b <= 64), "blocked", "multifrontal" or, on a mesh, "mesh_multifrontal": the route
// blocked_solve takes for effective tensors
const char* blocked_route_name(const BlockedWorkspace* ws);
const char* blocked_route_detail(BlockedWorkspace* ws);
// the route blocked_solve takes when correctors are asked for: the tree route's name where they stay on it, else "blocked"
const char* blocked_corrector_route_name(const BlockedWorkspace* ws);
// Load solves by substitution on the kept fronts (HOMMX_FLAG_TREE_LOADS / HOMMX_MESH_FLAG_TREE_LOADS; multifrontal.hip, mf_load_correctors).
// blocked_enable_tree_loads: ask for it when the plan is created -- it takes effect where the correctors stay on the tree, nowhere else;
// blocked_tree_loads: whether it did; blocked_load_route_name: "multifrontal_subst" / "mesh_multifrontal_subst" then, else the name
// blocked_corrector_route_name returns
void blocked_enable_tree_loads(BlockedWorkspace* ws);
bool blocked_tree_loads(const BlockedWorkspace* ws);
const char* blocked_load_route_name(const BlockedWorkspace* ws);
// cells per arena chunk of the corrector plan for batches of n_cells: builds and reserves that plan if need be, so that the rule "a chunk
// that ends in a load solve is at most one arena chunk" has its answer before the first solve; 0: the reservation failed (the solve
// that follows reports why)
long long blocked_tree_load_chunk(BlockedWorkspace* ws, long long n_cells);
// the correctors [cell][t][ndof] of the loads `lo` (rows l < n_loads, the rest zero) of the nc cells whose canonical corrector pass was the
// last call of blocked_solve with correctors: nothing is eliminated again; HOMMX_EINVAL when the arena does not hold exactly these cells
int blocked_load_correctors(BlockedWorkspace* ws, long long nc, const LoadOverride& lo, const double* d_M, double* d_corr_l, hipStream_t stream);
// dense flops one micro-cell solve executes on this route, by the route's own model (multifrontal: sum over the fronts of
// s^3 + 2 s^2 r + s r^2 on the padded sizes; plane elimination: (6 (n - 1) + 2) b^3)
double blocked_flops_per_cell(const BlockedWorkspace* ws);
}  // namespace hommx
