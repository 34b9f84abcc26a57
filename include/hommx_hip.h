/*
 * hommx_hip.h -- C ABI of libhommx_hip.so: the MI355X (gfx950) batched micro-cell solver that
 * replaces the per-macro-cell loop of flxrcz/hommx.
 *
 * The reference has no FFI layer; its seam is Python:
 *
 *   BaseHMM._assemble_stiffness()            src/hommx/hmm.py:298-332   loop over owned macro cells
 *     -> _compute_local_stiffness(cell)      src/hommx/hmm.py:334-369   nb corrector solves + nb^2 energies
 *          -> PeriodicLinearProblem.solve()  src/hommx/cell_problem.py:363-388
 *
 * This library replaces the LOOP: one call computes the effective tensor A_H / C_H of every macro
 * cell of a batch; the Python host (hommx_amd/hmm.py) turns it into S_loc = vol(T) G A_H G^T and
 * scatters on the CPU exactly where the reference calls MatSetValues (hmm.py:325-330).
 *
 * All arrays are C-contiguous, float64 / int32.  Plain pointers and sizes only; no torch types.
 * Every function returns 0 on success or a negative HOMMX_E* code; hommx_last_error() returns a
 * thread-local message.  Numerical failures are reported per cell in info[] (the reference logs
 * and continues: hmm.py:320-323, 427-430), never by the return code.
 */
#ifndef HOMMX_HIP_H
#define HOMMX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HOMMX_OK 0
#define HOMMX_EINVAL (-1)   /* bad argument / unsupported configuration */
#define HOMMX_EHIP (-2)     /* HIP runtime error (message in hommx_last_error) */
#define HOMMX_ENODEV (-3)   /* no usable GPU */
#define HOMMX_ENOMEM (-4)   /* device allocation failed */
#define HOMMX_ERCCL (-5)    /* RCCL error (message in hommx_last_error) */

/* problem kinds: which bilinear form of hmm.py the plan assembles */
#define HOMMX_KIND_POISSON_SCALAR 0     /* hmm.py:644-667 (and :759-789 when M != NULL); coef[cell][el]            */
#define HOMMX_KIND_POISSON_MATRIX 1     /* same forms, matrix-valued A; coef[cell][el][d(d+1)/2] (00,11,[22,]01[,02,12]) */
#define HOMMX_KIND_ELASTICITY_ISO 2     /* hmm.py:887-922 (and :1024-1067 when M != NULL); coef[cell][el][2]=(lambda,mu) */
#define HOMMX_KIND_ELASTICITY_VOIGT 3   /* same forms, full Hooke tensor; coef[cell][el][t(t+1)/2], upper triangle of
                                           the t x t matrix  E^m : A : E^n  (tensorial unit strains), row-major */

#define HOMMX_FLAG_FORCE_BLOCKED 1     /* use the generic blocked kernel family even where the fused 2D kernel applies */
#define HOMMX_FLAG_TREE_LOADS 4        /* a plan of the nested-dissection route ("multifrontal") does its load solves by substitution on
                                          the fronts the canonical pass of the chunk has just left in the corrector plan's arena
                                          ("multifrontal_subst", hommx_plan_load_kernel_name) instead of a second elimination; a chunk is
                                          then at most one arena chunk of that plan.  Off by default; accepted and without effect on every
                                          other route (and with HOMMX_MF_CORR=0).  Same bit as HOMMX_MESH_FLAG_TREE_LOADS */

/* Environment knobs (development / tuning; read once, when a plan is created):
 *   HOMMX_BLOCKED_MEM_GB   workspace budget of the blocked family in GB (default: plane elimination min(64, half of the free HBM),
 *                          nested dissection min(64 -- 128 through hommx_plan_reserve --, 0.6 x free HBM): its fronts are 0.2 GB per C4 / C5 cell)
 *   HOMMX_GEMM128_MIN      smallest M, N routed to the 128x128-tile GEMM (default 256 on the plane elimination; nested-dissection plans
 *                          use the 64x64 tiles throughout)
 *   HOMMX_TILE_SB          big lower-triangle updates walk their tiles in SB x SB super-blocks (default 4; 0: row by row)
 *   HOMMX_NO_SMALL_FUSED   any value: plane blocks b <= 64 take the HBM-resident kernels instead of the one-launch kernels
 *   HOMMX_MF_MIN_B         smallest plane block b routed to the nested-dissection (multifrontal) elimination instead of the plane
 *                          elimination (default: 65 in 3D, 49 in 2D, i.e. every plane block the one-launch kernels do not take or lose
 *                          on; 0: never; a value below 65 from the environment needs HOMMX_NO_SMALL_FUSED as well)
 *   HOMMX_MF_FRONT         most 16 x 16 tiles per dimension of a front that is eliminated by the register-resident front kernel
 *                          (csrc/mf_front_kernel.h: one launch per tree level) instead of the build / inverse / GEMM launch sequence
 *                          (default and maximum 19; 0: never)
 *   HOMMX_MF_STREAMS       1: the nested-dissection route runs on the caller's stream alone (default 4: every chunk as two to four pieces side
 *                          by side on the caller's stream and plan-owned ones; the caller's stream waits for all, results are bitwise equal)
 *   HOMMX_MF_CORR          0: hommx_solve_batch_correctors of a nested-dissection plan runs the plane elimination (default: back substitution
 *                          down the elimination tree on a second plan whose fronts all stay resident); HOMMX_FLAG_TREE_LOADS then has
 *                          no effect: there are no kept fronts to substitute on
 *   HOMMX_MF_LEAF, HOMMX_MF_SPLIT_DEPTH, HOMMX_MF_VERBOSE   tuning / A-B knobs of that route
 *   HOMMX_SMALL_WAVES      2 / 4: plane blocks b <= 48 take the LDS-resident multi-wave kernel (that many waves per macro cell)
 *                          instead of the one-wave-per-cell register kernel; for 48 < b <= 64 it sets that kernel's wave count
 *                          (2 / 4 / 8, default 8)
 *   HOMMX_RECON_MEM_MB     correctors hommx_reconstruct_batch[_device] holds on the device at once, in MB (default 1024): the batch runs in
 *                          chunks of that many cells' correctors; a fused 2D plan's factor records (HOMMX_FUSED_CORR) count with them
 *   HOMMX_FUSED_CORR       0: the correctors of a fused 2D plan come from the plane elimination of the blocked family (a blocked workspace
 *                          on first use).  Default: substitution on the block inverses of the fused kernel itself (k_poisson2d_fused<NB, true>
 *                          keeps them, k_fused2d_subst substitutes): two launches per chunk
 *   HOMMX_FUSED_LOADS      0: the load solve of hommx_loads_source[_device] on a fused 2D plan runs the plane elimination of the blocked family
 *                          (a blocked workspace on first use); implied by HOMMX_FUSED_CORR=0.  Default: substitution on the factor records of
 *                          the chunk's canonical pass (k_fused2d_subst_rhs): no second elimination.  Kept for A/B runs        */

typedef struct hommx_plan hommx_plan;

typedef struct hommx_plan_desc {
  int32_t dim;      /* 2 or 3 (hmm.py:104-105)                                                    */
  int32_t n_micro;  /* micro cells per side of the unit-cell mesh create_unit_square/cube(n,n[,n]) */
  int32_t kind;     /* HOMMX_KIND_*                                                                */
  int32_t device;   /* HIP device ordinal                                                          */
  int32_t flags;    /* HOMMX_FLAG_* bits, normally 0                                               */
  int32_t reserved[3];
} hommx_plan_desc;

/* Number of visible HIP devices (0 if none / runtime unusable). */
int hommx_device_count(void);

/* Create / destroy a plan = everything that does not depend on the batch: kernel selection,
 * stencil tables, device scratch.  Replaces the per-solve object construction of hmm.py:420-425
 * (dolfinx_mpc.LinearProblem.__init__: sparsity pattern + Mat + Vec + KSP for EVERY rhs of EVERY cell). */
int hommx_plan_create(hommx_plan** out, const hommx_plan_desc* desc);
int hommx_plan_destroy(hommx_plan* plan);

/* Optional: allocate the plan's device workspace for batches of up to n_cells now instead of in the first solve.  The nested-dissection
 * route of the C4 / C5 problem size holds ~0.2 GB of fronts per cell of a chunk: a first solve allocates up to min(64 GB, 0.6 x free HBM),
 * this call up to 128 GB (2 % more throughput over many batches) -- 2 to 6 s of hipMalloc that a benchmark wants outside its timed
 * region.  The fused 2D family keeps no workspace: a no-op there. */
int hommx_plan_reserve(hommx_plan* plan, int64_t n_cells);

/* Shape queries: elements per micro mesh (2 n^2 / 6 n^3), coefficient doubles per element,
 * t = size of the effective tensor (d for Poisson, d(d+1)/2 for elasticity), the descriptor fields, and the name of the
 * kernel route the plan's effective-tensor solves take: "fused2d" (2D scalar Poisson, n <= 32), "small_wave" (plane block
 * b <= 48: one wavefront per cell), "small_fused" (3D meshes with 48 < b <= 64: LDS), "multifrontal" (plane blocks b > 64 and 2D meshes with b > 48, e.g. 3D elasticity
 * from 5^3 micro cells: nested dissection, batched fronts) or "blocked" (everything else: plane elimination; also the corrector entry point of the small-block plans, see hommx_plan_corrector_kernel_name);
 * mesh plans: "mesh_front" or "mesh_multifrontal". */
int32_t hommx_plan_dim(const hommx_plan* plan);
int32_t hommx_plan_device(const hommx_plan* plan);
int32_t hommx_plan_n_micro(const hommx_plan* plan);
int32_t hommx_plan_kind(const hommx_plan* plan);
int64_t hommx_plan_num_elements(const hommx_plan* plan);
int32_t hommx_plan_coef_components(const hommx_plan* plan);
int32_t hommx_plan_tensor_size(const hommx_plan* plan);
const char* hommx_plan_kernel_name(const hommx_plan* plan);
/* The route the plan's corrector and reconstruction calls take: "fused2d_subst" (fused 2D plans; "blocked" with HOMMX_FUSED_CORR=0),
 * "multifrontal" / "mesh_multifrontal" (nested-dissection plans; "blocked" with HOMMX_MF_CORR=0 on a structured one), "mesh_front"
 * (frontal mesh plans), "blocked" (every other plan: plane elimination). */
const char* hommx_plan_corrector_kernel_name(const hommx_plan* plan);
/* The route the load solve of hommx_loads_source[_device] takes (the response outputs; P_eff alone needs none): "fused2d_subst" (fused 2D
 * plans; "blocked" with HOMMX_FUSED_LOADS=0 or HOMMX_FUSED_CORR=0), "mesh_front_subst" (frontal mesh plans created with HOMMX_MESH_FLAG_LOADS:
 * substitution on the pivot columns of the corrector arena), "none" (frontal mesh plans without the flag: the response is refused),
 * "multifrontal_subst" / "mesh_multifrontal_subst" (nested-dissection plans created with HOMMX_FLAG_TREE_LOADS / HOMMX_MESH_FLAG_TREE_LOADS
 * whose correctors stay on the tree: forward and backward substitution on the kept fronts of the chunk's canonical pass), else the name
 * hommx_plan_corrector_kernel_name returns. */
const char* hommx_plan_load_kernel_name(const hommx_plan* plan);
/* One line describing what that route launches for THIS plan (kernel names with their tile sizes, tree shape of the nested dissection,
 * stage size, streams): for reports -- bench.py's roofline.kernel label is this string, so it cannot drift from the code. */
const char* hommx_plan_route_detail(hommx_plan* plan);
/* Dense flops ONE micro-cell solve executes on the plan's route, by the route's own model: block-cyclic plane
 * elimination (6 (n-1) + 2) b^3; multifrontal: sum over the fronts of s^3 + 2 s^2 r + s r^2 on the padded front sizes. */
double hommx_plan_flops_per_solve(const hommx_plan* plan);

/*
 * Solve a batch of macro cells (host pointers; the call copies in, runs, copies out, synchronises).
 *
 *   coef   [n_cells][n_el][n_comp]  element means of A(c_T, y) (hmm.py:190-198, 349-352) in the element
 *                                   order  el = n_sub*(i + n*j [+ n*n*k]) + s  of the DOLFINx-style mesh
 *   M      [n_cells][d][d] or NULL  Dtheta_transpose(c_T), M[i][j] = d theta_j / d x_i (hmm.py:741, 756-757)
 *   A_eff  [n_cells][t][t]          out: effective tensor = vol(Y)^-1 * the functional of hmm.py:652-667 /
 *                                   774-789 / 905-922 / 1050-1067 on the canonical unit gradients / strains
 *   info   [n_cells] or NULL        out: 0 ok; k>0 non-positive or NaN pivot first seen in block step k-1 of the plane elimination
 *                                   (fused2d / small_* / blocked routes), or in the k-th group of fronts, counted from the leaves, of
 *                                   the multifrontal route; the cell's tensor is then not meaningful (the reference logs and goes on)
 */
int hommx_solve_batch(hommx_plan* plan, int64_t n_cells, const double* coef, const double* M,
                      double* A_eff, int32_t* info);

/* Same with DEVICE pointers, asynchronous on `stream` (a hipStream_t, NULL = default stream).  What that means, here and for every
 * other *_device entry point below (the stream-order contract; tests/test_gpu_stream_order.py pins it):
 *   - the call only queues work.  The inputs are read, and the outputs and the plan's scratch written, in the order of `stream`: behind
 *     everything queued on `stream` before the call (an input may still be in flight there when the call is made), and before anything
 *     queued on it afterwards (a later command on `stream` may read the outputs, overwrite the inputs or free them in stream order);
 *   - work the plan puts on streams of its own (the pieces of a nested-dissection chunk, HOMMX_MF_STREAMS) starts behind everything
 *     queued on `stream` before the call, and `stream` continues only behind all of that work;
 *   - a call may block the host while it grows the plan's scratch (a first call, a larger batch: hipFree / hipMalloc); it never
 *     waits for its own work, so the caller synchronises `stream`, or orders against it, before reading an output on the host or on
 *     another stream.
 * The library keeps no caller pointer beyond the work this call has queued: the arrays must stay valid until that work has run (free
 * them in stream order or after a synchronise, not on return).  The blocked and small-block kernel families work out of scratch the
 * PLAN owns (workspace, expanded coefficient stream): a plan is not thread-safe, and two calls on the same plan must not be in flight on
 * different streams at once (distinct plans are independent; the fused 2D family keeps no scratch beyond the factor records of its
 * corrector route). */
int hommx_solve_batch_device(hommx_plan* plan, int64_t n_cells, const double* d_coef, const double* d_M,
                             double* d_A_eff, int32_t* d_info, void* stream);

/*
 * Two-phase media sampled on the device ("on-device coefficient samplers").  Every BASELINE.json
 * configuration has a coefficient of the form  A(x, y) = indicator(y) ? a_1(x) : a_0(x)  (laminate.py:101-102,
 * inclusion.py:107-118, rotated_fibers.py:23-38): the fast variable only selects a phase.  Instead of streaming
 * n_el samples per macro cell the caller passes the phase mask ONCE and two values per cell:
 *
 *   mask    [n_el] uint8            phase of every micro element (element order of the DOLFINx-style mesh)
 *   values  [n_cells][2][n_comp]    coefficient of phase 0 / phase 1 at the macro cell midpoint c_T
 *
 * The fused 2D kernel selects in registers (no coefficient stream at all: 16 bytes per cell instead of 16 KiB); the
 * blocked family expands into its scratch stream on the device.  Host pointers; same outputs as hommx_solve_batch.
 */
int hommx_solve_batch_two_phase(hommx_plan* plan, int64_t n_cells, const uint8_t* mask, const double* values,
                                const double* M, double* A_eff, int32_t* info);

/* Same with DEVICE pointers, asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract). */
int hommx_solve_batch_two_phase_device(hommx_plan* plan, int64_t n_cells, const uint8_t* d_mask, const double* d_values,
                                       const double* d_M, double* d_A_eff, int32_t* d_info, void* stream);

/*
 * Separable coefficients sampled on the device.  The smooth coefficients of the reference's own tests are a
 * slow amplitude times a fixed function of the fast variable:  A(x, y) = a(x) + b(x) g(y)  (test_integration_poisson.py:149-150,
 * 197: 0.33 + 0.15 (sin 2 pi x0 + sin 2 pi y0); :268: 1.1 + x0 + sin 2 pi y0)  or its reciprocal  1 / (a(x) + b(x) g(y))
 * (:124-125: 1 / (2 + cos 2 pi y0)).  g is tabulated ONCE on the micro mesh at the points of the quadrature rule UFL would pick
 * (degree 3: 6 points per triangle); the kernels form the element means from (a, b) of each macro cell, so 16 bytes per cell
 * cross the boundary instead of n_el samples.  Scalar Poisson kind; isotropic elasticity kind with one (a, b) pair per Lame
 * parameter and the same g (test_integration_linear_elasticity.py:78-93: lambda = 1.25, mu = 5 + 4.5 sin 2 pi y0).
 *
 *   family   HOMMX_SAMPLER_AFFINE      A_K = a + b * table[K]                      table[n_el] = sum_q w_q g(y_{K,q})
 *            HOMMX_SAMPLER_RECIPROCAL  A_K = sum_q weights[q] / (a + b * table[K][q])   table[n_el][n_q] = g(y_{K,q})
 *   params   [n_cells][n_comp][2] = (a, b) of every coefficient component at the macro cell midpoint c_T (n_comp = 1, or 2 = (lambda, mu))
 *
 * Every operation is a separately rounded IEEE-754 operation in the written order (q ascending), so a host evaluating the same
 * formula reproduces the element stream bit for bit (hommx_amd.hmm.Separable.host_stream; tests/test_gpu_separable.py).
 */
#define HOMMX_SAMPLER_AFFINE 0
#define HOMMX_SAMPLER_RECIPROCAL 1
int hommx_solve_batch_separable(hommx_plan* plan, int64_t n_cells, int32_t family, int32_t n_q, const double* table,
                                const double* weights, const double* params, const double* M, double* A_eff, int32_t* info);

/* Same with DEVICE pointers, asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract). */
int hommx_solve_batch_separable_device(hommx_plan* plan, int64_t n_cells, int32_t family, int32_t n_q, const double* d_table,
                                       const double* d_weights, const double* d_params, const double* d_M, double* d_A_eff,
                                       int32_t* d_info, void* stream);

/* Same as hommx_solve_batch, additionally returning the correctors (host pointers):
 *   correctors [n_cells][t][n^d * bs]  chi_m of the canonical load case m (unit gradient e_m / unit strain E^m) at the
 *                                      periodic unknowns, dof = node * bs + component, node = i + n j [+ n^2 k];
 *                                      mean-free per component (the reference removes the constants: cell_problem.py:349-361).
 * These are the functions the reference keeps in self._correctors (hmm.py:204-207, 431) / PoissonPeriodicHMM.correctors
 * (hmm.py:1211-1213, 1239-1240), for the canonical loads instead of the nb macro basis functions: the corrector of a
 * macro basis function is the linear combination  eps * sum_m (grad phi_i)_m chi_m  (SURVEY A.2, row A5).
 * Route: plans whose tensors take the nested-dissection route get the correctors by back substitution down the same elimination tree
 * (a second plan of that tree whose fronts all stay resident; HOMMX_MF_CORR=0: plane elimination); a fused 2D plan runs its elimination
 * once more with the block inverses kept and substitutes on them (k_fused2d_subst; HOMMX_FUSED_CORR=0: plane elimination), in chunks of
 * HOMMX_RECON_MEM_MB of factor records and correctors; every other plan runs the plane elimination of the blocked family here (the
 * one-launch kernels never form the factors).  hommx_plan_corrector_kernel_name names the route. */
int hommx_solve_batch_correctors(hommx_plan* plan, int64_t n_cells, const double* coef, const double* M,
                                 double* A_eff, double* correctors, int32_t* info);

/*
 * HMM reconstruction: the micro fields inside the sampling box of every macro cell, from the macro solution.
 * For macro cell c with macro gradient / strain xi[c] (t entries: grad u_H|_T for the Poisson kinds; for elasticity the Voigt vector of
 * eps(u_H)|_T with doubled shear, (e00, e11[, e22], 2 e01[, 2 e02, 2 e12])) and the canonical correctors chi_m of the cell (the layout of
 * hommx_solve_batch_correctors), chi^xi = sum_m xi_m chi_m and, for every micro element K (volume |K|, P1 gradients g_a, periodic nodes p_a):
 *   s_K = xi + sum_a sum_alpha chi^xi[p_a bs + alpha] strain(g_a, M, alpha)   gradient / strain in the canonical-load basis (shear doubled)
 *   q_K = material(coef_K) s_K                                                flux A grad R (no sign flip) / stress (s00, s11[, s22], s01[, s02, s12])
 *   stats[c] = [ sum |K| s_K (t) | sum |K| q_K (t) | sum |K| s_K . q_K | max_K |q_K| | smallest K reaching the max (as a double) ]
 * |q| is the Euclidean norm for Poisson, the Frobenius norm of the stress (shear entries counted twice) for elasticity.  Exactly, on the
 * discrete problem: mean strain = xi, mean flux = A_eff xi, energy = xi . A_eff xi (Hill-Mandel).  A cell's stats do not depend on its batch
 * position, the chunking or whether fields are written (fixed-order reduction).
 *
 *   coef, M          as hommx_solve_batch                      strain, flux  [n_cells][n_el][t] or both NULL: per-element fields
 *   xi               [n_cells][t]                              A_eff, info   as hommx_solve_batch, or NULL
 *   stats            [n_cells][HOMMX_RECON_NSTATS(t)], required
 * Every plan: the structured routes (a fused 2D plan forms the correctors from its own factors, as
 * hommx_solve_batch_correctors) and both mesh routes.  The batch runs in chunks: the correctors of one chunk, with the factor records of a
 * fused 2D plan (HOMMX_RECON_MEM_MB), live in plan-owned scratch, never the whole batch's; the host entry also streams coef in and the outputs out chunk by chunk.
 */
#define HOMMX_RECON_NSTATS(t) (2 * (t) + 3) /* [mean_strain(t) | mean_flux(t) | energy | max_flux | argmax_element] */
int hommx_reconstruct_batch(hommx_plan* plan, int64_t n_cells, const double* coef, const double* M, const double* xi, double* stats,
                            double* strain, double* flux, double* A_eff, int32_t* info);
/* Same with DEVICE pointers, asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract); the plan's scratch is shared with its other entry points (not thread-safe). */
int hommx_reconstruct_batch_device(hommx_plan* plan, int64_t n_cells, const double* d_coef, const double* d_M, const double* d_xi,
                                   double* d_stats, double* d_strain, double* d_flux, double* d_A_eff, int32_t* d_info, void* stream);

/*
 * Reconstruction from a coefficient in any of the four forms the solve entry points take, with optional per-region statistics.  The
 * sampler forms send a few numbers per macro cell (hommx_solve_batch_two_phase / _separable) and are expanded into the plan's element
 * stream on the device, chunk by chunk (the smaller of HOMMX_RECON_MEM_MB of correctors and 1 GiB of stream): the stream the host would
 * form, bit for bit, so every output equals hommx_reconstruct_batch's on that stream.  Only the pointers of `form` are read:
 *
 *   HOMMX_COEF_SAMPLED     coef    [n_cells][n_el][n_comp]                     as hommx_solve_batch
 *   HOMMX_COEF_TWO_PHASE   mask    [n_el] uint8, values [n_cells][2][n_comp]   as hommx_solve_batch_two_phase
 *   HOMMX_COEF_SEPARABLE   family, n_q, table, weights, params [n_cells][n_comp][2]   as hommx_solve_batch_separable, with its
 *                          restrictions on family and kind
 *   HOMMX_COEF_PROGRAM     program, n_q, table [n_el][n_q][dim], weights [n_q], params [n_cells][3]   an expression, see hommx_coef_program
 *
 * Regions: region[n_el] (uint8) labels every micro element; with n_regions = R > 0 the call also returns, per cell and region r < R,
 *   region_stats[c][r] = [ volume | sum |K| s_K (t) | sum |K| q_K (t) | sum |K| s_K . q_K | max |q_K| | smallest K reaching it ]
 * over the elements K with region[K] == r.  The sums are NOT divided by the volume.  An element whose label is >= R belongs to no region
 * (this is how a caller leaves elements out; labels are not validated).  An empty region reports volume 0, sums 0, max = -1 and
 * argmax = -1, the values the whole-cell reduction starts from.  Each region is reduced by the code and in the order of the whole-cell
 * statistics, so the largest regional max equals stats' max bitwise when the regions cover the cell, and a region's statistics do not
 * depend on batch position, chunking or fields either.  n_regions == 0: region and region_stats are NULL.  n_regions >
 * HOMMX_RECON_MAX_REGIONS, or a non-zero n_regions without both pointers, is HOMMX_EINVAL -- but HOMMX_COEF_TWO_PHASE with n_regions == 2
 * and region == NULL takes the mask as the labels (region 0: phase 0, region 1: phase 1).
 * stats, strain, flux, A_eff, info, M, xi: as hommx_reconstruct_batch.  The host entry sends mask / table / weights / labels and the
 * per-cell values in one pinned block owned by the plan; a sampled stream goes in, and every output comes back, chunk by chunk.
 */
#define HOMMX_COEF_SAMPLED 0
#define HOMMX_COEF_TWO_PHASE 1
#define HOMMX_COEF_SEPARABLE 2
#define HOMMX_COEF_PROGRAM 3

/*
 * Expression coefficients sampled on the device: A(x, y) as a postfix program over a stack of doubles, interpreted by a hand-written
 * kernel (csrc/coef_program.hip) -- the program is data, nothing is compiled at run time.  With the source's
 *   table    [n_el][n_q][dim]   the points y_{K,q} of the micro quadrature rule on every micro element
 *   weights  [n_q]              its weights,  n_q >= 1 their number
 *   params   [n_cells][3 + n_fields]   the midpoint c_T of every macro cell (x of the expression), then the cell's fields
 * the element mean of component c is  A_K[c] = sum_q weights[q] * v_c(c_T, y_{K,q}),  accumulated as acc = acc + weights[q] * v from 0
 * with q ascending, every operation of the program and of the sum one separately rounded IEEE-754 operation in the written order: a
 * host that interprets the same program (hommx_amd.expr.Expression.host_stream) reproduces the element stream bit for bit when the
 * program holds exactly rounded operations only (everything but SQRT .. TANH below), and to the accuracy of the device's math
 * functions otherwise.  The stream is expanded into the plan's scratch chunk by chunk (at most 1 GiB) on EVERY
 * plan -- a fused 2D plan then runs the mode that reads a sampled stream -- so every output equals the one of that stream, bit for bit.
 *
 * ops[n_ops][2] = (opcode, operand); the operand is the index of CONST / X / Y / STORE and ignored otherwise:
 *    0 CONST k  push consts[k]      1 X i  push x[i], i < 3; field i - 3, 3 <= i < 3 + n_fields      2 Y i  push y[i], i < dim
 *    3 ADD  4 SUB  5 MUL  6 DIV     (a, b) -> a op b, b on top
 *    7 NEG  8 ABS                   9 MIN  10 MAX  (a, b) -> b < a ? b : a  /  b > a ? b : a
 *   11 LT  12 LE  13 GT  14 GE      (a, b) -> 1.0 or 0.0         15 AND  16 OR  17 NOT  on "non-zero is true", -> 1.0 or 0.0
 *   18 SELECT   (c, a, b) -> c != 0 ? a : b  (both evaluated)
 *   19 SQRT  20 SIN  21 COS  22 TAN  23 EXP  24 LOG  25 TANH      26 DUP      27 STORE c  pop the value of component c
 * Validation (HOMMX_EINVAL with a text naming the fault, on the host, before the plan's device is made current): a null program, ops
 * or consts, n_q < 1, null table / weights / params; n_ops outside 1 .. 128, n_consts outside 0 .. 32; n_comp other than the plan's;
 * a plan of the HOMMX_KIND_ELASTICITY_VOIGT kind (21 components: not supported); an unknown opcode; a CONST, X or Y index out of range;
 * stack underflow; stack depth above 16; a component stored twice or never; values left on the stack at the end; n_params outside
 * 0 .. HOMMX_PROGRAM_MAX_PARAMS or above n_consts; the source's n_fields outside 0 .. HOMMX_PROGRAM_MAX_FIELDS; an X index at or above
 * 3 + n_fields.
 *
 * Parameters: the first n_params constants are the parameters p[0 .. n_params-1] of the expression, shared by all macro cells.  For
 * the solve, expand, reconstruct and loads entries they are constants like the others, and n_params == 0 is a program without
 * parameters on every path.  hommx_expand_tangents differentiates the program with respect to them, and HOMMX_DIRS_PARAMETERS makes
 * those derivatives the directions of the derivative entries.
 *
 * Fields: hommx_coef_source.n_fields (0 .. HOMMX_PROGRAM_MAX_FIELDS) values PER MACRO CELL -- a design variable, the macro solution at
 * the midpoint, a random draw -- which stand after the midpoint in the cell's row of `params` and are read by `X k`, k >= 3, like a
 * coordinate of the midpoint.  No entry point, opcode or struct is added for them: the member was `reserved` (0), so a caller that
 * never heard of fields passes a program without them, and everything about such a source is what it was.  The kernels load a field
 * where it is read (the row stays in cache) instead of holding it in a register.  The differentiable slots of hommx_expand_tangents and
 * HOMMX_DIRS_PARAMETERS are the parameters, then the fields: n_tan = n_params + n_fields, at most HOMMX_PROGRAM_MAX_PARAMS together;
 * the derivative with respect to a field is the derivative of the cell's stream with respect to the cell's OWN value.
 */
#define HOMMX_PROGRAM_MAX_PARAMS 4
#define HOMMX_PROGRAM_MAX_FIELDS 4
typedef struct hommx_coef_program {
  int32_t n_ops, n_consts, n_comp;
  int32_t n_params;      /* 0 .. HOMMX_PROGRAM_MAX_PARAMS, <= n_consts (this member was `reserved`, 0) */
  const uint8_t* ops;    /* [n_ops][2]: opcode, operand */
  const double* consts;  /* [n_consts]                  */
} hommx_coef_program;

typedef struct hommx_coef_source {
  int32_t form;     /* HOMMX_COEF_*                                    */
  int32_t family;   /* HOMMX_SAMPLER_* (HOMMX_COEF_SEPARABLE)          */
  int32_t n_q;      /* columns of table (HOMMX_SAMPLER_RECIPROCAL)     */
  int32_t n_fields; /* HOMMX_COEF_PROGRAM: fields per macro cell, 0 .. HOMMX_PROGRAM_MAX_FIELDS; read for that form ONLY (this member was
                       `reserved`, 0) */
  const double* coef;
  const uint8_t* mask;
  const double* values;
  const double* table;
  const double* weights;
  const double* params;
  const hommx_coef_program* program; /* HOMMX_COEF_PROGRAM: host memory in the device entries too; read for that form ONLY, so a caller
                                        built against the struct that ended with params is never read past its end */
} hommx_coef_source;

/* The generic twin of hommx_solve_batch / _two_phase / _separable: a coefficient source in any form (hommx_reconstruct_source lists
 * them; only the pointers of `form` are read), M, A_eff and info as hommx_solve_batch.  The host entry sends the small arrays of a
 * sampler form in one pinned block owned by the plan (a sampled stream goes the way of hommx_solve_batch). */
int hommx_solve_batch_source(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* M, double* A_eff, int32_t* info);
/* Same with DEVICE pointers (in *src as well; the structs themselves are host memory), asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract). */
int hommx_solve_batch_source_device(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* d_M, double* d_A_eff,
                                    int32_t* d_info, void* stream);
/* The element stream a source expands to: coef_out[n_cells][n_el][n_comp], what hommx_solve_batch would be given (a sampled source is
 * copied).  For checking a sampler against its host equivalent, and for callers that want the stream itself. */
int hommx_expand_source(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, double* coef_out);
/* Same with DEVICE pointers (in *src as well), asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract). */
int hommx_expand_source_device(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, double* d_coef_out, void* stream);

/*
 * The derivatives of the element stream of a HOMMX_COEF_PROGRAM source with respect to its parameters and its fields (the n_tan =
 * n_params + n_fields differentiable slots, the parameters first; 1 <= n_tan <= HOMMX_PROGRAM_MAX_PARAMS), in forward mode: ONE pass of
 * the interpreter (csrc/coef_program.hip, k_expand_program<P>; the value pass is its P = 0) carries (v, d_0 .. d_{P-1}) per stack
 * entry and yields
 *   coef_out [n_cells][n_el][n_comp]             the stream of hommx_expand_source, bit for bit (or NULL: not wanted)
 *   dirs_out [n_cells][n_tan][n_el][n_comp]      d coef / d slot j (p[j], or field j - n_params of the cell itself), the layout of
 *                                                per-cell directions (hommx_sens_args, per_cell == 1)
 * Every arithmetic step is one separately rounded IEEE-754 operation in the written order, no contraction; hommx_amd.expr.Expression
 * .host_tangents applies the same rules in the same order with NumPy.  For parameter j, if every operand's d_j is 0.0 the result's d_j
 * is +0.0 and the formula is not evaluated: a sqrt(0) or a division by zero in a part of the expression that does not depend on p[j]
 * cannot make its tangent NaN.  Otherwise, for operands (a, da), (b, db), b on top, and the instruction's own value v:
 *   CONST k   d_j = (k == j && k < n_params) ? 1 : 0           X k, k < 3, Y   d_j = 0           DUP   copies
 *   X k, k >= 3:   d_j = (j == n_params + k - 3) ? 1 : 0
 *   ADD  da + db         SUB  da + (-db)         NEG  -da
 *   MUL  add(mul(a, db), mul(da, b))             DIV  div(add(da, -mul(v, db)), b),  v = a / b
 *   ABS  a < 0 ? -da : da          MIN / MAX / SELECT  the tangent of the operand the value rule picks
 *   LT .. GE, AND, OR, NOT  0      (a parameter inside a comparison moves an interface: its derivative is zero almost everywhere)
 *   SQRT div(da, mul(2, v))        SIN  mul(cos(a), da)        COS  -mul(sin(a), da)        TAN  mul(da, add(1, mul(v, v)))
 *   EXP  mul(v, da)                LOG  div(da, a)             TANH mul(da, add(1, -mul(v, v)))
 *   STORE c   acc[c] = add(acc[c], mul(w, v));  accd[c][j] = add(accd[c][j], mul(w, d_j)),  q ascending, from 0
 * Validation: that of hommx_expand_source, and HOMMX_EINVAL with a text for a source of another form, n_tan == 0, n_tan above
 * HOMMX_PROGRAM_MAX_PARAMS (the text names both counts), a null dirs_out.
 * The host entry stages the source as hommx_expand_source does and returns chunk by chunk (at most 1 GiB of the 1 + n_tan streams).
 */
int hommx_expand_tangents(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, double* coef_out, double* dirs_out);
/* Same with DEVICE pointers (in *src as well), asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract). */
int hommx_expand_tangents_device(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, double* d_coef_out, double* d_dirs_out,
                                 void* stream);

/*
 * The second derivatives of that element stream with respect to the same n_tan slots, in SECOND-ORDER forward mode: the interpreter
 * (csrc/coef_program.hip, k_expand_program2<P>, the same body as k_expand_program<P>) carries (v, d_a, d_b, h_aa, h_ab, h_bb) per stack
 * entry -- (v, d, h) for one slot -- and yields, beside the two streams of hommx_expand_tangents,
 *   curv_out [n_cells][n_pairs][n_el][n_comp]    d2 coef / d slot a d slot b for the pairs (a, b), a <= b, in row-major order:
 *                                                (0,0), (0,1), .., (0,n_tan-1), (1,1), ..;  n_pairs = n_tan (n_tan + 1) / 2.  Required
 *   coef_out, dirs_out                           as in hommx_expand_tangents, the same bits; either may be NULL: not wanted
 * n_tan <= 2 is one pass; n_tan = 3, 4 runs the two-slot pass once per pair of slots a < b (3 or 6 launches), each launch storing
 * the streams no earlier one has stored.  Every arithmetic step is one separately rounded operation in the written order, no
 * contraction; hommx_amd.expr.Expression.host_second_tangents applies the same rules in the same order with NumPy.  For operands
 * (a, da, ha), (b, db, hb), b on top, the instruction's own value v and its own tangents d (the rules above), h = h_ij of the result:
 * if every operand's h_ij is 0.0 and every operand's d_i, or every operand's d_j, is 0.0, the result's h_ij is +0.0 and the formula
 * is not evaluated (a sqrt(0) or a division by zero in a part that does not read both slots cannot make it NaN).  Otherwise
 *   CONST, X, Y   0          DUP  copies          LT .. GE, AND, OR, NOT   0
 *   ADD  add(ha, hb)         SUB  add(ha, -hb)    NEG  -ha          ABS  a < 0 ? -ha : ha
 *   MUL  add(add(add(mul(a, hb), mul(ha, b)), mul(da_i, db_j)), mul(da_j, db_i))
 *   DIV  div(add(add(add(ha, -mul(d_i, db_j)), -mul(d_j, db_i)), -mul(v, hb)), b)
 *   MIN / MAX / SELECT  the h of the operand the value rule picks
 *   SQRT div(add(ha, -mul(mul(2, d_i), d_j)), mul(2, v))
 *   SIN  add(mul(cos(a), ha), -mul(mul(v, da_i), da_j))        COS  add(-mul(sin(a), ha), -mul(mul(v, da_i), da_j))
 *   TAN  add(mul(g, ha), mul(mul(mul(2, v), d_j), da_i)),  g = add(1, mul(v, v))
 *   TANH add(mul(g, ha), -mul(mul(mul(2, v), d_j), da_i)), g = add(1, -mul(v, v))
 *   EXP  add(mul(v, ha), mul(d_j, da_i))                       LOG  div(add(ha, -mul(da_i, d_j)), a)
 *   STORE c   acch[c][ij] = add(acch[c][ij], mul(w, h_ij)),  q ascending, from 0
 * Validation: that of hommx_expand_tangents, with a null curv_out in the place of a null dirs_out.  The host entry stages and
 * chunks as hommx_expand_tangents does (at most 1 GiB of the 1 + n_tan + n_pairs streams).
 */
int hommx_expand_second_tangents(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, double* coef_out, double* dirs_out,
                                 double* curv_out);
/* Same with DEVICE pointers (in *src as well), asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract). */
int hommx_expand_second_tangents_device(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, double* d_coef_out, double* d_dirs_out,
                                        double* d_curv_out, void* stream);

#define HOMMX_RECON_MAX_REGIONS 8
#define HOMMX_RECON_NREGION(t) (2 * (t) + 4) /* [volume | sum strain(t) | sum flux(t) | energy | max_flux | argmax_element] */
int hommx_reconstruct_source(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* M, const double* xi,
                             int32_t n_regions, const uint8_t* region, double* stats, double* region_stats, double* strain, double* flux,
                             double* A_eff, int32_t* info);
/* Same with DEVICE pointers (in *src as well; the struct itself is host memory), asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract). */
int hommx_reconstruct_source_device(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* d_M, const double* d_xi,
                                    int32_t n_regions, const uint8_t* d_region, double* d_stats, double* d_region_stats, double* d_strain,
                                    double* d_flux, double* d_A_eff, int32_t* d_info, void* stream);

/*
 * Derivatives of A_H along coefficient directions.  Let s^m_K be the gradient / strain of micro element K under
 * the canonical load xi = e_m (the s_K of hommx_reconstruct_batch: shear doubled, M applied) and material(c) the element operator of the
 * plan's kind, which is linear in the coefficient components for all four kinds.  For any perturbation dir[K][q] of the element stream,
 * exactly on the discrete problem,
 *   dA[c][d][m][n] = sum_K |K| s^m_K . material(dir_d[K]) s^n_K
 * -- no derivative of a corrector appears (the cell equation makes those terms vanish), the gauge does not matter, and A_H being
 * 1-homogeneous in the coefficient, the direction dir = coef gives dA = A_eff (Euler).  With weights w[c][t][t] the call also returns the
 * per-element gradient of the functional w : A_H,
 *   grad[c][K][q] = |K| sum_{m,n} w[c][m][n] s^m_K . material(e_q) s^n_K        (e_q: the unit coefficient vector of component q)
 * so that sum_{K,q} grad[c][K][q] dir[K][q] = sum_{m,n} w[c][m][n] dA[dir][c][m][n].
 *
 *   n_dirs      0 .. HOMMX_SENS_MAX_DIRS direction streams, each shaped like one cell's coefficient [n_el][n_comp]
 *   per_cell    0: dirs[n_dirs][n_el][n_comp], shared by all cells; 1: dirs[n_cells][n_dirs][n_el][n_comp];
 *               HOMMX_DIRS_PARAMETERS: the directions are the derivatives of the source's program with respect to its parameters and fields
 *               (hommx_expand_tangents), formed on the device chunk by chunk in the launch that expands the stream, into plan-owned
 *               scratch whose bytes the chunk rule counts: dirs == NULL, n_dirs == n_tan = the program's n_params + the source's
 *               n_fields (1 .. HOMMX_PROGRAM_MAX_PARAMS), dA as with per_cell == 1.
 *               HOMMX_EINVAL with a text for a source that is no HOMMX_COEF_PROGRAM, n_tan == 0 or above 4, another n_dirs, a non-null dirs;
 *               and for HOMMX_DIRS_PARAMETERS_CURVATURE, which hommx_sens2_args alone takes (a first derivative has no curvature term)
 *   dA          [n_cells][n_dirs][t][t] (symmetric, bitwise); required with n_dirs > 0, as dirs
 *   weights     [n_cells][t][t] and grad [n_cells][n_el][n_comp] (the shape of coef): both or neither
 *   A_eff, info as hommx_solve_batch, or NULL
 * src, M: as hommx_reconstruct_source.  HOMMX_EINVAL, before the plan's device is made current: a null plan, source or argument struct,
 * n_dirs out of range, n_dirs > 0 without both dirs and dA, one of weights / grad without the other, nothing requested (n_dirs == 0 and
 * no grad).  Every plan is accepted; the correctors of one chunk (HOMMX_RECON_MEM_MB, the chunk rule of the reconstruction) live in
 * plan-owned scratch.  A cell's outputs do not depend on its batch position, the chunking or which outputs are requested (fixed-order
 * reduction).  A cell whose elimination flags a pivot keeps its info; its outputs may hold anything, no other cell's change.  The host
 * entry sends shared directions with the source's shared arrays once; per-cell directions, weights and a sampled stream go in, and
 * every output comes back, chunk by chunk.
 */
#define HOMMX_SENS_MAX_DIRS 8
#define HOMMX_DIRS_PARAMETERS 2 /* a value of per_cell in hommx_sens_args and hommx_sens2_args */
#define HOMMX_DIRS_PARAMETERS_CURVATURE 3 /* a value of per_cell in hommx_sens2_args only: d2A takes the curvature term as well */
typedef struct hommx_sens_args {
  int32_t n_dirs;
  int32_t per_cell;
  const double* dirs;
  double* dA;
  const double* weights;
  double* grad;
  double* A_eff;
  int32_t* info;
} hommx_sens_args;
int hommx_sensitivity_source(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* M, const hommx_sens_args* args);
/* Same with DEVICE pointers (in *src and *args as well; the structs themselves are host memory), asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract). */
int hommx_sensitivity_source_device(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                    const hommx_sens_args* args, void* stream);

/*
 * Derivatives of A_H with respect to the stratification M.  M = Dtheta^T(c_T) enters a cell problem only through
 * the strain of a local dof, which is linear in it: with H^n_K[alpha][b] = sum_a chi_n[p_a bs + alpha] g_a[b] the raw gradient of the
 * canonical corrector n on micro element K (no M), s^n_K = e_n + voigt(H^n_K M^T) is the s^n_K of hommx_sensitivity_source (shear doubled)
 * and sigma^n_K = material(coef_K) s^n_K its flux / stress (Poisson: the vector q^n[a]; elasticity: the symmetric d x d tensor of the Voigt
 * vector, shear NOT doubled).  C0 does not depend on M, and exactly on the discrete problem
 *   dA_dM[c][a][b][m][n] = sum_K |K| [ (sigma^m_K H^n_K)[a][b] + (sigma^n_K H^m_K)[a][b] ]         (Poisson: q^m[a] h^n[b] + q^n[a] h^m[b])
 * -- no derivative of a corrector appears (the cell equation makes those terms vanish) and the gauge does not matter.  A_H being
 * 0-homogeneous in M (scaling M rescales the correctors), sum_{a,b} M[a][b] dA_dM[c][a][b] = 0 (Euler).  With weights w[c][t][t] the call
 * also returns the adjoint product
 *   grad_M[c][a][b] = sum_{m,n} w[c][m][n] dA_dM[c][a][b][m][n]
 * in one pass and without the t x t intermediate: d d numbers per cell instead of d d t t (w = xi_v (x) xi_u: the derivative of the
 * energy density xi_v . A_H xi_u).
 *
 *   dA_dM       [n_cells][d][d][t][t] (symmetric in (m, n), bitwise), or NULL
 *   weights     [n_cells][t][t] and grad_M [n_cells][d][d]: both or neither
 *   A_eff, info as hommx_solve_batch, or NULL
 * src, M: as hommx_reconstruct_source; M == NULL differentiates at M = I.  HOMMX_EINVAL, before the plan's device is made current: a null
 * plan, source or argument struct, one of weights / grad_M without the other, nothing requested (neither dA_dM nor grad_M).  Every plan
 * is accepted; the correctors of one chunk (HOMMX_RECON_MEM_MB, the chunk rule of the reconstruction) live in plan-owned scratch.  A
 * cell's outputs do not depend on its batch position, the chunking or which outputs are requested (fixed-order reduction).  A cell whose
 * elimination flags a pivot keeps its info; its outputs may hold anything, no other cell's change.  The host entry sends a sampled stream,
 * M and the weights in, and every output back, chunk by chunk.
 */
typedef struct hommx_strat_sens_args {
  double* dA_dM;
  const double* weights;
  double* grad_M;
  double* A_eff;
  int32_t* info;
} hommx_strat_sens_args;
int hommx_stratification_sensitivity_source(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* M,
                                            const hommx_strat_sens_args* args);
/* Same with DEVICE pointers (in *src and *args as well; the structs themselves are host memory), asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract). */
int hommx_stratification_sensitivity_source_device(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                                   const hommx_strat_sens_args* args, void* stream);

/*
 * User-supplied polarisation loads of the cell problem: a prescribed micro flux / stress field P(y), such as a
 * thermal eigenstress -A : alpha dT, a prestress, the gravity term of Darcy flow or the residual of a Newton step.  Per macro cell the
 * caller gives n_loads fields P^l[n_el][t], constant per micro element, components in the order of hommx_reconstruct_batch's flux
 * (Poisson: the flux vector; elasticity: s00, s11[, s22], s01[, s02, s12], shear NOT doubled).  With eps(z)_K the strain of a periodic
 * field z on element K (shear doubled, M applied, as s_K of hommx_reconstruct_batch) and chi^m the canonical correctors, exactly on the
 * discrete problem:
 *   corrector      a(chi_l, z) = -sum_K |K| P^l_K . eps(z)_K  for all z                 (P^l = material(coef) e_m gives chi_l = chi^m)
 *   total flux     q^l_K       = P^l_K + material(coef_K) eps(chi_l)_K
 *   P_eff[c][l]    = sum_K |K| q^l_K = sum_K |K| (e_m + eps(chi^m)_K) . P^l_K, m < t       (Levin: from the canonical correctors alone)
 *   energy[c][l][l'] = sum_K |K| eps(chi_l)_K . material(coef_K) eps(chi_l')_K              (symmetric, bitwise)
 * P_eff is all a macro solve needs (its load gains -vol(T) eps_macro(v) . P_eff); it is computed by the Levin form, which needs no
 * second elimination, on EVERY plan.  The response outputs come from a solve for the loads themselves (hommx_plan_load_kernel_name names
 * its route): a fused 2D plan substitutes on the factor records its canonical pass has just left (k_fused2d_subst_rhs; with
 * HOMMX_FUSED_LOADS=0 it gets a blocked workspace on the first such call instead), every other plan runs one more corrector pass of the
 * blocked family with the load rows replaced (a mesh plan of the tree route among them); a frontal mesh plan substitutes on the pivot
 * columns its canonical pass has just left in the corrector arena (k_mesh_front_rhs) when it was created with HOMMX_MESH_FLAG_LOADS.
 * A plan of a nested-dissection route created with HOMMX_FLAG_TREE_LOADS / HOMMX_MESH_FLAG_TREE_LOADS substitutes on the fronts its
 * canonical pass has just left in the corrector plan's arena instead (forwards up the tree on a row block of all fronts, backwards by
 * the back substitution of the canonical correctors); a chunk is then at most one arena chunk of that plan (HOMMX_BLOCKED_MEM_GB).
 *
 *   n_loads     1 .. t of the plan (callers loop for more)
 *   per_cell    a code: where the load comes from, alone or or-ed with the flag HOMMX_LOADS_EIGENSTRAIN
 *               HOMMX_LOADS_SHARED (0): P[n_loads][n_el][t], shared by all cells; HOMMX_LOADS_PER_CELL (1): P[n_cells][n_loads][n_el][t]
 *               HOMMX_LOADS_PROGRAM (2): P is not read (NULL); the load is sampled on the device from P_source, a HOMMX_COEF_PROGRAM
 *               source of the load's OWN beside the coefficient's: its own program with n_comp == t (the components of P in their
 *               order), its own table (points), weights and n_q, its own params rows [n_cells][3 + n_fields] and n_fields.  n_loads
 *               must be 1 (callers loop for more).  Per chunk the rows of its cells are expanded by the value pass of the interpreter
 *               into plan-owned scratch, [cell][el][comp] = P[cell][0][el][:], and every consumer reads that as a per-cell load.  The
 *               rounding contract of a program holds word for word: separately rounded operations in the written order, acc = acc +
 *               w[q] v with q ascending from 0, so the load is bit for bit the per-cell array a host interpreter of the same program
 *               forms.  Everything a HOMMX_COEF_PROGRAM coefficient source is checked for is checked of P_source, against t
 *               components (and on every kind, HOMMX_KIND_ELASTICITY_VOIGT included)
 *               HOMMX_LOADS_EIGENSTRAIN (4, a flag): what the array or the program delivers is an eigenstrain E^l_K[t] -- a thermal
 *               strain alpha dT, a swelling, a misfit -- in the components and convention of hommx_reconstruct_batch's strain
 *               (Poisson: a gradient; elasticity: e00, e11[, e22], then DOUBLED shears), and the load is the eigenstress
 *               P^l_K = -material(coef_K) E^l_K, formed on the device (k_eigenstress) from the element stream of the call's
 *               coefficient source, whatever its form, before anything reads P.  A shared E becomes a per-cell P (the coefficient
 *               differs per cell) in plan-owned scratch, as does the caller's per-cell E of the device entry, which is left as it
 *               is; the expansion of a program and the chunk of a per-cell E a host call has sent are overwritten in place
 *   P_source    read ONLY when (per_cell & 3) == HOMMX_LOADS_PROGRAM: a caller built against the struct that ended with `info` and
 *               passes codes 0 and 1 is never read past its end
 *   P_eff       [n_cells][n_loads][t], required
 *   A_eff, info of the canonical pass, as hommx_solve_batch, or NULL
 *   response, every one optional, any of them triggers the load solve:
 *   energy      [n_cells][n_loads][n_loads]
 *   stats       [n_cells][n_loads][t+2] = [sum |K| q^l_K (t) | max_K |q^l_K| | smallest K reaching it]; norms and rule of
 *               hommx_reconstruct_batch (Frobenius for elasticity); the first t equal P_eff up to rounding (two independent paths)
 *   strain, flux [n_cells][n_loads][n_el][t]: eps(chi_l)_K and q^l_K; both or neither
 *   correctors  [n_cells][n_loads][ndof], mean-free per component, dof order of hommx_solve_batch_correctors
 * src, M: as hommx_reconstruct_source.  HOMMX_EINVAL, before the plan's device is made current: a null plan, source or argument struct,
 * n_loads out of range, an unknown code in per_cell (a bit beyond 7, or (per_cell & 3) == 3), a null P (codes without HOMMX_LOADS_PROGRAM)
 * or P_eff, for HOMMX_LOADS_PROGRAM a null P_source, one of another form, n_loads != 1, a program whose n_comp is not t and everything
 * else a program source is refused for, one of strain / flux without the other.  HOMMX_EINVAL as well, before any work: a response output on a
 * plan of the frontal mesh route created without HOMMX_MESH_FLAG_LOADS ("mesh_front" builds its loads in the basis of the canonical ones;
 * with the flag the load solve substitutes on its pivot columns, and a chunk then also holds them: HOMMX_RECON_MEM_MB counts the arena,
 * and a chunk is at most one arena chunk; HOMMX_MESH_FLAG_TREE, the tree route, serves these too).  The correctors of
 * one chunk (HOMMX_RECON_MEM_MB, the chunk rule of the reconstruction; a response holds two blocks of t correctors per cell) live in
 * plan-owned scratch.  A cell's outputs do not depend on its batch position, the chunking or which outputs are requested (fixed-order
 * reductions).  A cell whose elimination flags a pivot keeps its info; no other cell's outputs change.  The host entry sends a shared P
 * with the source's shared arrays once; a per-cell P and a sampled stream go in, and every output comes back, chunk by chunk.
 * The points, weights and rows of P_source travel with the source's shared arrays too (the device entry takes device pointers in
 * *P_source as in *src; both structs and the program are host memory and are read before it returns).  What the device forms of the load
 * for a chunk (n_el t doubles per cell for a program, n_loads n_el t for an eigenstrain array it may not overwrite) counts in the chunk
 * rule, and the expansion of a program in the 1 GiB bound of the expanded streams.
 */
#define HOMMX_LOADS_SHARED 0
#define HOMMX_LOADS_PER_CELL 1
#define HOMMX_LOADS_PROGRAM 2     /* P is NULL; the load comes from P_source */
#define HOMMX_LOADS_EIGENSTRAIN 4 /* flag, or-ed to any of the three: what arrives is an eigenstrain E, P = -material(coef) E */
typedef struct hommx_load_args {
  int32_t n_loads;
  int32_t per_cell;
  const double* P;
  double* P_eff;
  double* A_eff;
  double* energy;
  double* stats;
  double* strain;
  double* flux;
  double* correctors;
  int32_t* info;
  const hommx_coef_source* P_source; /* read only when (per_cell & 3) == HOMMX_LOADS_PROGRAM */
} hommx_load_args;
int hommx_loads_source(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* M, const hommx_load_args* args);
/* Same with DEVICE pointers (in *src and *args as well; the structs themselves are host memory), asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract). */
int hommx_loads_source_device(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                              const hommx_load_args* args, void* stream);

/*
 * Second derivatives of A_H along coefficient directions, exact on the discrete problem.  With s^m_K,
 * material() and the directions of hommx_sensitivity_source, and eps(z)_K the strain of a periodic field z as in hommx_loads_source: the
 * derivative of the canonical corrector m along dir_b is the corrector of a polarisation load,
 *   K chi^m_b = -f(P^{b,m}),  P^{b,m}_K = material(dir_b[K]) s^m_K                        (the load convention of hommx_loads_source)
 *   g_ab[m][n] = sum_K |K| eps(chi^m_b)_K . material(dir_a[K]) s^n_K
 *   d2A[c][a][b][m][n] = g_ab[m][n] + g_ab[n][m] = d^2 A_H[m][n] / d theta_a d theta_b     (coef + theta_a dir_a + theta_b dir_b)
 * -- the element operator is linear in the stream, so no second derivative of it appears.  d2A is symmetric in (m, n) and in (a, b),
 * both bitwise (every block is formed once and mirrored); d2A[a][a] is negative semidefinite (A_H is concave in the coefficient); A_H
 * being 1-homogeneous, every block with the cell's own coefficient as one of its directions vanishes up to rounding (Euler).  The call
 * costs one canonical corrector pass and one load solve per direction (hommx_plan_load_kernel_name names its route: a fused 2D plan
 * substitutes on the factor records the canonical pass has just left, a frontal mesh plan with HOMMX_MESH_FLAG_LOADS on the pivot
 * columns of its corrector arena, every other plan runs one more corrector pass of the blocked family) against the 2 n_dirs + 1 eliminations of central differences of hommx_sensitivity_source.
 *
 *   n_dirs      1 .. HOMMX_SENS_MAX_DIRS
 *   per_cell    0: dirs[n_dirs][n_el][n_comp], shared by all cells; 1: dirs[n_cells][n_dirs][n_el][n_comp];
 *               HOMMX_DIRS_PARAMETERS: the parameter tangents of the source's program, as in hommx_sens_args (dirs == NULL, n_dirs ==
 *               n_params).  d2A then holds the second derivatives ALONG THE TANGENT DIRECTIONS.  For a program that is affine in its
 *               parameters that is the Hessian of A_H with respect to them; for any other the Hessian also needs dA_H along
 *               d2 coef / dp_a dp_b, the curvature term, which this value leaves out;
 *               HOMMX_DIRS_PARAMETERS_CURVATURE: the arguments and checks of HOMMX_DIRS_PARAMETERS, and the launch that expands the
 *               chunk is the second-order pass (hommx_expand_second_tangents): it also forms the n_pairs second-order streams, in
 *               plan-owned scratch whose bytes the chunk rule counts; k_sens contracts them into dA_H[kappa_ab] ([n_pairs][t][t]
 *               per cell, scratch too) and d2A[a][b] = add(d2A[a][b], dA_H[kappa_ab]) for every (a, b), (b, a) with the addend of
 *               (a, b): d2A is then the HESSIAN of A_H in the parameters and fields for any program, still symmetric bitwise in
 *               (a, b) and (m, n).  dA, A_eff and info are exactly those of HOMMX_DIRS_PARAMETERS
 *   d2A         [n_cells][n_dirs][n_dirs][t][t], required
 *   dA          [n_cells][n_dirs][t][t] or NULL: the first derivatives along the same directions, the bits hommx_sensitivity_source returns
 *   A_eff, info as hommx_solve_batch, or NULL
 * src, M: as hommx_reconstruct_source.  HOMMX_EINVAL, before the plan's device is made current: a null plan, source or argument struct,
 * n_dirs out of range, a null dirs or d2A, and a plan of the frontal mesh route created without HOMMX_MESH_FLAG_LOADS ("mesh_front" has no load
 * solve then: create the plan with that flag, or with HOMMX_MESH_FLAG_TREE, the tree route).  Every other plan is accepted.  Per cell of a chunk (HOMMX_RECON_MEM_MB, the chunk rule of the
 * reconstruction) plan-owned scratch holds two blocks of t correctors and the t loads of one direction (t n_el t doubles).  A cell's
 * outputs do not depend on its batch position, the chunking or which optional outputs are requested (fixed-order reductions).  A cell
 * whose elimination flags a pivot keeps its info; its outputs may hold anything, no other cell's change.  The host entry sends shared
 * directions with the source's shared arrays once; per-cell directions, a sampled stream and M go in, and every output comes back,
 * chunk by chunk.
 */
typedef struct hommx_sens2_args {
  int32_t n_dirs;
  int32_t per_cell;
  const double* dirs;
  double* d2A;
  double* dA;
  double* A_eff;
  int32_t* info;
} hommx_sens2_args;
int hommx_second_sensitivity_source(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* M, const hommx_sens2_args* args);
/* Same with DEVICE pointers (in *src and *args as well; the structs themselves are host memory), asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract). */
int hommx_second_sensitivity_source_device(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                           const hommx_sens2_args* args, void* stream);

/*
 * Failure criteria on the reconstructed micro state.  With e_K the gradient / strain and q_K the flux / stress
 * of micro element K as hommx_reconstruct_batch forms them from xi and the canonical correctors -- and, with a load, the total state
 * under the macro strain plus the load, e_K + eps(chi_P)_K and q_K + P_K + material(coef_K) eps(chi_P)_K of hommx_loads_source --, one
 * scalar program is interpreted once per element,
 *   v_K = program(row of the element),  row = [midpoint (3) | fields (n_fields) | e_K (t) | q_K (t) | coef_K (n_comp)],
 * and only its statistics come back.  The program is a hommx_coef_program with n_comp == 1 (one STORE 0) in the opcodes of
 * HOMMX_COEF_PROGRAM, none added: the state is read like a field, `X k` with k = 3 + n_fields + j for e[j], 3 + n_fields + t + j for
 * q[j] and 3 + n_fields + 2 t + j for coef[j]; `Y i` is coordinate i of the element's centroid, points[K][i].  Every operation is one
 * separately rounded IEEE operation in program order (value pass only; hommx_amd.expr.Criterion.host_values interprets the same program
 * with NumPy), and e_K, q_K are formed without contraction, so v_K does not depend on which outputs are asked for.
 *
 *   program     n_comp == 1; host memory in the device entry too
 *   n_fields    0 .. HOMMX_PROGRAM_MAX_FIELDS fields of the criterion's own per macro cell; rows [n_cells][3 + n_fields]
 *   points      [n_el][dim], shared by all cells; may be NULL if the program has no Y
 *   xi          [n_cells][t], as hommx_reconstruct_batch
 *   threshold   the value from which an element counts into crit[3]; not NaN
 *   has_load    0: the mechanical state alone (per_cell, P and P_source are not read).  Else ONE load (n_loads == 1 of hommx_load_args)
 *               with the codes and the meaning of hommx_load_args.per_cell, HOMMX_LOADS_EIGENSTRAIN included: HOMMX_LOADS_PER_CELL with
 *               P[n_cells][n_el][t], or HOMMX_LOADS_PROGRAM with P_source.  HOMMX_LOADS_SHARED is refused (points is the call's one
 *               shared array: a caller repeats a shared load per cell).  The chunk is then that of a response of hommx_loads_source:
 *               the load solve on the route hommx_plan_load_kernel_name names, a second corrector block per cell
 *   crit        [n_cells][4] = [max_K v_K | the smallest K reaching it | sum |K| v_K | sum |K| [v_K >= threshold]], required.  A NaN
 *               v_K never wins the maximum (-inf and -1 when every element is NaN) and makes the sum NaN
 *   values      [n_cells][n_el] = v_K, or NULL
 *   strain, flux [n_cells][n_el][t] = e_K, q_K, the totals the program saw; both or neither
 *   A_eff, info of the canonical pass, as hommx_solve_batch, or NULL
 * src, M: as hommx_reconstruct_source.  HOMMX_EINVAL, before the plan's device is made current: a null plan, source, argument struct,
 * program, rows, xi or crit; one of strain / flux without the other; n_fields out of range; everything a program is refused for
 * (hommx_coef_program) against n_comp == 1 and a row of 3 + n_fields + 2 t + n_comp entries, on every kind; a Y in the program with
 * points NULL; a NaN threshold; with has_load the refusals of hommx_loads_source for its code and P / P_source, and
 * HOMMX_LOADS_SHARED.  HOMMX_EINVAL as well, before any work: has_load on a plan of the frontal mesh route created without
 * HOMMX_MESH_FLAG_LOADS.  The correctors of one chunk (HOMMX_RECON_MEM_MB) live in plan-owned scratch.  Per workgroup the kernel holds
 * the field in LDS beside 4 KiB per stack level below the top; a cell for which that exceeds the limit of the reconstruction keeps the
 * field in a scratch slot, which the chunk rule counts.  The statistics of a cell do not depend on its batch position, the chunking or
 * which outputs are requested (fixed-order reductions).  A cell whose elimination flags a pivot keeps its info; its outputs may hold
 * anything, no other cell's change.
 */
typedef struct hommx_criterion_args {
  const hommx_coef_program* program;
  int32_t n_fields;
  const double* rows;
  const double* points;
  const double* xi;
  double threshold;
  int32_t has_load, per_cell;
  const double* P;
  const hommx_coef_source* P_source; /* read only when has_load and (per_cell & 3) == HOMMX_LOADS_PROGRAM */
  double* crit;
  double* values;
  double* strain;
  double* flux;
  double* A_eff;
  int32_t* info;
} hommx_criterion_args;
#define HOMMX_CRIT_NSTATS 4
int hommx_criterion_source(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* M, const hommx_criterion_args* args);
/* Same with DEVICE pointers (in *src, *args and *args->P_source as well; the structs and the programs are host memory), asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract). */
int hommx_criterion_source_device(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                  const hommx_criterion_args* args, void* stream);

/*
 * Strain-dependent coefficients: the secant (Kacanov) iteration of a cell, on the device.  A law is a
 * hommx_coef_program in the opcodes of HOMMX_COEF_PROGRAM, none added, on the row of a criterion,
 *   row = [midpoint (3) | fields (n_fields) | e_K (t) | s_K (t) | c_K (n_comp)],
 * with n_comp == the plan's: one STORE k per entry of the element's coefficient, on every kind (the 21 Voigt entries included).
 * c_K is the BASE coefficient of the element, the stream `src` expands to; e_K the gradient / strain of the current iterate and
 * s_K = material(current coefficient of K) e_K its secant flux / stress.  `Y i` is coordinate i of the element's centroid.
 *
 * Cell T starts from c^0 = coef_start (if given) or the base stream.  Round j = 0, 1, ...:
 *   1. the correctors and A^j = A_eff(c^j) on the plan's route;
 *   2. per element e_K, q_K = material(c^j_K) e_K, formed without contraction as hommx_criterion_source forms them;
 *   3. v_K = law(row), n_comp values; w_K = v_K if relax == 1, else add_rn(mul_rn(1 - relax, c^j_K), mul_rn(relax, v_K));
 *   4. change^j = max_{K,k} |w - c^j| / max_{K,k} |w| (0 when both are 0), mean_flux^j = sum_K |K| q_K (fixed-order reductions);
 *   5. the cell stops with a status, tested in this order -- 3: info[T] != 0, the elimination flagged a pivot (change and mean_flux
 *      are then NaN, the law is not evaluated); 2: some v_K is not finite; 0: change^j <= tol; 1: j + 1 == max_iter -- or goes on
 *      with c^{j+1} = w.
 * The outputs are those of the stopping round and belong together: A_eff = A^j, mean_flux, coef_out = c^j (the stream A_eff belongs
 * to: a stopping round never commits w), state = [rounds = j + 1 | change^j | status], and strain / flux / law_values of that round.
 * A stopped cell is frozen: its stream is not touched again, so the later eliminations of its chunk reproduce its A_eff and info bit
 * for bit, and its outputs do not depend on its neighbours, its batch position, the chunking, max_iter beyond its own stopping round,
 * the outputs asked for or the entry point.
 *
 *   program     n_comp == the plan's; host memory in the device entry too
 *   n_fields    0 .. HOMMX_PROGRAM_MAX_FIELDS fields of the law's own per macro cell; rows [n_cells][3 + n_fields]
 *   points      [n_el][dim], shared by all cells; may be NULL if the program has no Y
 *   xi          [n_cells][t]
 *   max_iter    >= 1;  tol >= 0, not NaN;  relax in (0, 1]
 *   coef_start  [n_cells][n_el][n_comp] or NULL
 *   state       [n_cells][3], required;  A_eff [n_cells][t][t], required;  mean_flux [n_cells][t] or NULL
 *   coef_out    [n_cells][n_el][n_comp] or NULL
 *   strain, flux [n_cells][n_el][t], both or neither;  law_values [n_cells][n_el][n_comp] = v_K or NULL
 *   info        as hommx_solve_batch, or NULL
 * src, M: as hommx_reconstruct_source.  A load beside the law: hommx_secant_load_source.  HOMMX_EINVAL, before the plan's device is made current: a null plan,
 * source, argument struct, program, rows, xi, state or A_eff; one of strain / flux without the other; everything a program is refused
 * for against n_comp == the plan's and a row of 3 + n_fields + 2 t + n_comp entries; a Y in the program with points NULL; max_iter
 * < 1; tol negative or NaN; relax outside (0, 1].  The chunk is that of the reconstruction, with the current and the candidate stream
 * of a chunk (2 n_el n_comp doubles per cell) counted as scratch.  The device entry queues exactly max_iter rounds per chunk and
 * reads nothing back; the host entry reads the chunk's state after each round and stops when no cell runs.  Both give the same bits.
 */
typedef struct hommx_secant_args {
  const hommx_coef_program* program;
  int32_t n_fields;
  const double* rows;
  const double* points;
  const double* xi;
  int32_t max_iter;
  double tol, relax;
  const double* coef_start;
  double* state;
  double* A_eff;
  double* mean_flux;
  double* coef_out;
  double* strain;
  double* flux;
  double* law_values;
  int32_t* info;
} hommx_secant_args;
#define HOMMX_SECANT_NSTATE 3
int hommx_secant_source(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* M, const hommx_secant_args* args);
/* Same with DEVICE pointers (in *src and *args; the structs and the program are host memory), asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract). */
int hommx_secant_source_device(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                               const hommx_secant_args* args, void* stream);

/*
 * The consistent tangent D = d sigma_H / d xi of the secant response, sigma_H(xi) = mean_flux, at the state the iteration stops in
 * (DESIGN.md section 4.16).  The law must be EXPLICIT: it reads e, c, x, y, p and f but no entry of s (an `X` index in
 * [3 + n_fields + t, 3 + n_fields + 2 t)).  With b_K the base coefficient and c_K = L(e_K, b_K) the converged one,
 *   T_K[m][n] = material(c_K)[m][n] + sum_k g_k[m] dL_k/de[n],   g_k = material(unit_k) e_K,
 * and D is A_eff of the LINEAR cell problem whose element coefficient is T_K, a full symmetric t x t matrix: a coefficient of
 * HOMMX_KIND_POISSON_MATRIX for the Poisson kinds and of HOMMX_KIND_ELASTICITY_VOIGT for the elasticity kinds (the tangent kind).
 * dL/de is the forward mode of the law over the strain, by the rules of hommx_expand_tangents, the dead rule included, accumulated
 * at each STORE k as T[m][n] = add_rn(T[m][n], mul_rn(g_k[m], d_k[n])) from material(c_K).  The elimination needs a symmetric
 * coefficient, and T_K is symmetric exactly when the law derives from a potential: the device writes the symmetric part
 * mul_rn(0.5, add_rn(T[m][n], T[n][m])) and reports asymmetry = max_K |T - T^T| / max_K |T| of the cell (0 when both are 0), so a
 * caller sees when D is the tangent of the symmetrised law only.
 *
 * Per chunk: the rounds of hommx_secant_source -- every output named in *secant has its bits --, one launch that forms the tangent
 * stream of the chunk from the correctors the last round left, and one hommx_solve_batch_device of that stream on tangent_plan with
 * the same M on the same stream.  A cell of status 2 or 3 gets the identity material in its tangent stream, asymmetry NaN and
 * tangent NaN.
 *
 *   secant        the iteration, exactly as hommx_secant_source takes it
 *   tangent_plan  a plan of the tangent kind with the dim, the micro mesh (n, or n_el and the nodes) and the device of `plan`; not `plan`
 *   tangent       [n_cells][t][t], required: D;  asymmetry [n_cells], required
 *   tangent_coef  [n_cells][n_el][t (t + 1) / 2] or NULL: the tangent stream, in the component order of the tangent kind
 *   tangent_info  [n_cells] or NULL: info of the tangent elimination
 * HOMMX_EINVAL, before the plan's device is made current: everything hommx_secant_source refuses; a null tangent_plan, tangent or
 * asymmetry; a tangent plan of another kind, dim, size or device, or `plan` itself; a program that reads an s entry.  The tangent
 * stream of a chunk (n_el t (t + 1) / 2 doubles per cell) counts as scratch of the chunk where tangent_coef is NULL.  The device
 * entry reads nothing back: max_iter rounds, one tangent launch and one solve per chunk; the host entry gives the same bits.
 */
typedef struct hommx_secant_tangent_args {
  const hommx_secant_args* secant;
  hommx_plan* tangent_plan;
  double* tangent;
  double* asymmetry;
  double* tangent_coef;
  int32_t* tangent_info;
} hommx_secant_tangent_args;
int hommx_secant_tangent_source(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* M,
                                const hommx_secant_tangent_args* args);
/* Same with DEVICE pointers (in *src, *args and *args->secant; the structs and the program are host memory), asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract). */
int hommx_secant_tangent_source_device(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                       const hommx_secant_tangent_args* args, void* stream);

/*
 * History variables of a law: 1 .. HOMMX_SECANT_MAX_HISTORY internal variables per micro element that
 * survive from one call to the next -- a damage driver, the largest field an element has seen.  The row of the law grows by them,
 *   row = [midpoint (3) | fields (n_fields) | e_K (t) | s_K (t) | c_K (n_comp) | h_K (n_history)],
 * and its program stores n_comp + n_history values (program->n_comp is that sum): STORE k, k < n_comp, is entry k of the coefficient
 * as before, STORE n_comp + i the UPDATE of h_i, the value history_out receives.  h_K is history_in of the element: the history at
 * the START of the call, read in every round and frozen for the whole iteration -- which is why history_in and history_out must not
 * be the same array.  The rounds are those of hommx_secant_source with these additions: an update that is not finite counts towards
 * status 2 as a component does; the history does not enter `change`; history_out belongs to the stopping round as A_eff, coef_out and
 * state do and is frozen with them; a cell that stops with status 2 or 3 gets history_out = history_in bit for bit.  The caller
 * decides when history_out becomes the state (it passes it as history_in of the next load step).
 *
 *   n_history    1 .. HOMMX_SECANT_MAX_HISTORY
 *   history_in   [n_cells][n_el][n_history], required
 *   history_out  [n_cells][n_el][n_history], required, not history_in
 * Every other argument is hommx_secant_source's, resp. hommx_secant_tangent_source's, and so is every output, the struct included.
 * The tangent entries differentiate the components at the frozen history (max(h, ...) has its loading and its unloading branch) on
 * the program truncated behind the last component's STORE -- the updates stand behind it and are not differentiated --, and their
 * law must read no s entry anywhere, the updates included.
 * HOMMX_EINVAL, before the plan's device is made current: everything the entry without history refuses, with the program checked
 * against n_comp + n_history components and a row of 3 + n_fields + 2 t + n_comp + n_history entries (its stores must be exactly
 * 0 .. n_comp + n_history - 1); a null history struct, history_in or history_out; n_history outside 1 .. HOMMX_SECANT_MAX_HISTORY;
 * history_in == history_out.  Both arrays are per-cell arrays of the chunk, counted as coef_start and coef_out are.  The device
 * entries read nothing back, so a caller can keep the history resident on the device.
 */
#define HOMMX_SECANT_MAX_HISTORY 4
typedef struct hommx_history_args {
  int32_t n_history;
  const double* history_in;
  double* history_out;
} hommx_history_args;
int hommx_secant_history_source(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* M,
                                const hommx_secant_args* args, const hommx_history_args* history);
/* Same with DEVICE pointers (in *src, *args and *history; the structs and the program are host memory), asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract). */
int hommx_secant_history_source_device(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                       const hommx_secant_args* args, const hommx_history_args* history, void* stream);
int hommx_secant_tangent_history_source(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* M,
                                        const hommx_secant_tangent_args* args, const hommx_history_args* history);
/* Same with DEVICE pointers, asynchronous on `stream`. */
int hommx_secant_tangent_history_source_device(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                               const hommx_secant_tangent_args* args, const hommx_history_args* history, void* stream);

/*
 * A load beside a law: the secant iteration with ONE polarisation or eigenstrain per cell (n_loads == 1),
 * solved for in every round.  The load comes per cell or as a program, in the codes of hommx_load_args.per_cell:
 *   per_cell    HOMMX_LOADS_PER_CELL (P[n_cells][n_el][t]) or HOMMX_LOADS_PROGRAM (P is not read; the load is sampled on the device
 *               from P_source, a HOMMX_COEF_PROGRAM source with n_comp == t, as hommx_load_args describes), alone or or-ed with
 *               HOMMX_LOADS_EIGENSTRAIN.  HOMMX_LOADS_SHARED is refused, as hommx_criterion_source refuses it.
 *   P           the polarisation P_K[t] (shear not doubled) or, with the flag, the eigenstrain E_K[t] (shear doubled)
 *   P_source    read only when (per_cell & 3) == HOMMX_LOADS_PROGRAM
 * Round j of cell T on its current stream c^j:
 *   1. with the flag only: the eigenstress of the round, P^j = -material(c^j) E, into scratch of the chunk.  The eigenstrain array is
 *      never overwritten -- every round and the round kernel read it --, a host call's staged array and the expansion of a program
 *      included; the chunk rule counts the extra field;
 *   2. the canonical correctors and A^j, as hommx_secant_source forms them;
 *   3. the corrector chi_P^j of the load on c^j, on the route hommx_plan_load_kernel_name names, behind the canonical block (the
 *      block layout and the chunk rule of hommx_criterion_source with a load);
 *   4. the round of hommx_secant_source on X = sum_m xi_m chi_m + chi_P^j, where the law reads
 *        a polarisation:  e[k] the total strain e_K, s[k] the total flux q_K = material(c^j_K) e_K + P_K, as a criterion sees it;
 *        an eigenstrain:  e[k] the elastic strain g_K = e_K - E_K (one rounded subtraction per component), s[k] q_K = material(c^j_K) g_K
 *      -- the model sigma = c(eps - eps*) (eps - eps*), which keeps a strain-driven law explicit.  The `strain` output is what e[k]
 *      read, `flux` is q_K, and mean_flux = sum |K| q_K.
 * The effective polarisation of the stopping state needs no output of its own: it is mean_flux - A_eff xi (Levin's identity).  The
 * tangent entries give D = d mean_flux / d xi unchanged in form, the effective tensor of the element tangents T_K, evaluated at the
 * strain the law saw (total or elastic).  Everything else is hommx_secant_source's, resp. hommx_secant_tangent_source's: the status
 * rules and frozen cells, commits on non-stopping rounds only, fixed-order reductions, the independence of chunking, batch position,
 * max_iter, the outputs asked for and the entry point; the device entries queue exactly max_iter rounds and read nothing back.
 * history: NULL for a law without history variables, else as the history entries take it.
 * HOMMX_EINVAL, before the plan's device is made current: everything the entry without a load refuses (with or without history); a
 * null load struct; an unknown code in per_cell; HOMMX_LOADS_SHARED; a null P for HOMMX_LOADS_PER_CELL; for HOMMX_LOADS_PROGRAM a null
 * P_source, one of another form, or a program whose n_comp is not t.  HOMMX_EINVAL as well, before any work: a plan of the frontal
 * mesh route created without HOMMX_MESH_FLAG_LOADS.
 */
typedef struct hommx_secant_load_args {
  int32_t per_cell;
  const double* P;
  const hommx_coef_source* P_source;
} hommx_secant_load_args;
int hommx_secant_load_source(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* M, const hommx_secant_args* args,
                             const hommx_history_args* history /* NULL: none */, const hommx_secant_load_args* load);
/* Same with DEVICE pointers (in *src, *args, *history, *load and *load->P_source; the structs and the programs are host memory), asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract). */
int hommx_secant_load_source_device(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                    const hommx_secant_args* args, const hommx_history_args* history, const hommx_secant_load_args* load,
                                    void* stream);
int hommx_secant_tangent_load_source(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* M,
                                     const hommx_secant_tangent_args* args, const hommx_history_args* history /* NULL: none */,
                                     const hommx_secant_load_args* load);
/* Same with DEVICE pointers, asynchronous on `stream`. */
int hommx_secant_tangent_load_source_device(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                            const hommx_secant_tangent_args* args, const hommx_history_args* history,
                                            const hommx_secant_load_args* load, void* stream);

/*
 * Criteria and reconstruction statistics of the NONLINEAR state: a second tail behind the secant iteration.
 * The rounds are exactly those of hommx_secant_load_source -- of hommx_secant_history_source or hommx_secant_source where `load` resp.
 * `history` is NULL --, and every output named in *args and *history has its bits.  After the last round of a chunk the tail runs,
 * per cell, on the stream coef_out describes, the corrector blocks of the last executed round (a stopped cell's elimination reproduces
 * them), the load array or the eigenstress of that round, the base stream and history_in.  It adds no elimination.
 *   crit_program  NULL: no criterion.  Else ONE component (n_comp == 1) on the row
 *                   [midpoint (3) | fields (crit_n_fields) | e_K (t) | s_K (t) | c_K (n_comp) | h_K (n_history) | b_K (n_comp)],
 *                 the row of a law with history with the base behind it: e_K the total strain, s_K = material(c_K) e_K + P_K the total
 *                 flux (P the polarisation or the eigenstress of the round), c_K the stream the iteration stopped on, h_K history_in
 *                 of the element (n_history == 0 without a history struct), b_K the base stream, what the law calls c[k].  `Y i`
 *                 reads args->points.
 *   crit_n_fields, crit_rows   the criterion's OWN fields, [n_cells][3 + crit_n_fields] (the law's rows stay args->rows)
 *   threshold, crit, crit_values   as hommx_criterion_args.threshold, .crit ([n_cells][HOMMX_CRIT_NSTATS], required with a program)
 *                 and .values ([n_cells][n_el] or NULL)
 *   total_strain, total_flux   [n_cells][n_el][t], both or neither: what the criterion saw
 *   reconstruct   != 0: stats [n_cells][HOMMX_RECON_NSTATS(t)] (required) and, with n_regions > 0, region / region_stats: the
 *                 statistics of hommx_reconstruct_source on the stopped state
 * For a program that reads neither b nor h, crit, crit_values, total_strain and total_flux are bit for bit what
 * hommx_criterion_source returns for coef_out as a per-cell stream with the same xi, M, rows, points and load; stats and region_stats
 * are bit for bit hommx_reconstruct_source's for coef_out.  A cell of status 0, 1 or 2 is evaluated on its c^j; a cell of status 3 keeps
 * its info, its tail outputs may hold anything, and no other cell's outputs change.  The tail outputs of a cell do not depend on its
 * batch position, the chunking, max_iter beyond its stopping round, the outputs asked for, or the entry point.  The chunk rule is the
 * underlying entry's with the per-cell tail outputs and crit_rows counted; the tail holds no scratch of its own.
 * HOMMX_EINVAL, before the plan's device is made current: everything the underlying entry refuses; a null state struct; neither a
 * program nor reconstruct; with a program everything hommx_criterion_source refuses for program, fields, rows, threshold, crit and one
 * of strain / flux alone, the program checked against a row of 3 + crit_n_fields + 2 t + 2 n_comp + n_history entries (an h index
 * without a history struct is out of that row's h segment); with reconstruct a null stats, the region refusals of
 * hommx_reconstruct_source, and reconstruct together with a load (the statistics have no load term: refused, not computed wrongly).
 */
typedef struct hommx_secant_state_args {
  const hommx_coef_program* crit_program;
  int32_t crit_n_fields;
  const double* crit_rows;
  double threshold;
  double* crit;
  double* crit_values;
  double* total_strain;
  double* total_flux;
  int32_t reconstruct;
  int32_t n_regions;
  const uint8_t* region;
  double* stats;
  double* region_stats;
} hommx_secant_state_args;
int hommx_secant_state_source(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* M, const hommx_secant_args* args,
                              const hommx_history_args* history /* NULL: none */, const hommx_secant_load_args* load /* NULL: none */,
                              const hommx_secant_state_args* state);
/* Same with DEVICE pointers (in *src, *args, *history, *load, *load->P_source and *state; the structs and the programs are host memory), asynchronous on `stream` (hommx_solve_batch_device: the stream-order contract): max_iter rounds and the tail are queued, nothing is read back. */
int hommx_secant_state_source_device(hommx_plan* plan, int64_t n_cells, const hommx_coef_source* src, const double* d_M,
                                     const hommx_secant_args* args, const hommx_history_args* history, const hommx_secant_load_args* load,
                                     const hommx_secant_state_args* state, void* stream);

/*
 * Unstructured periodic micro meshes.  Any simplicial mesh of the unit square / cube whose boundary is
 * periodic: the caller folds the mesh vertices into n_nodes independent (periodic) nodes -- cell_problem.py:38-300's slave -> master
 * map -- and passes, per element, the periodic node of every vertex and the UNFOLDED vertex coordinates (gradients and volumes).
 * The plan is a hommx_plan of one of two routes: "mesh_front" (batched frontal elimination, one workgroup per macro cell, the front in
 * LDS) for meshes whose frontal width is at most HOMMX_MESH_MAX_FRONT, and "mesh_multifrontal" (nested
 * dissection of the mesh by coordinate bisection, eliminated by the multifrontal engine of the structured routes) for wider meshes and
 * for any mesh with HOMMX_MESH_FLAG_TREE.  hommx_solve_batch[_device], _two_phase[_device], _separable[_device], _correctors,
 * hommx_plan_reserve, the accessors and hommx_plan_destroy take either unchanged (hommx_plan_n_micro is 0).
 * hommx_solve_batch_multi[_device] refuses both (HOMMX_EINVAL).
 *
 *   coef[cell][el]    follows the element order of the descriptor
 *   gauge             the last node of the elimination order is pinned (its bs unknowns dropped), as on the structured routes; on
 *                     the tree route the node of highest elimination rank in the root front (A_H does not depend on the choice)
 *   correctors        [n_cells][t][n_nodes * bs], dof = node * bs + component in the caller's node ids, mean-free per component
 *   info[cell]        k > 0: the k-th pivot (counted from 1 in elimination order) was non-positive or not finite
 *   flops_per_solve   sum over the pivots of f^2 + 2 f t, f = unknowns in the front at that pivot (itself included); on the tree
 *                     route the dense flops of the multifrontal model (padded fronts, as hommx_plan_flops_per_solve of the structured
 *                     multifrontal route)
 */
#define HOMMX_MESH_MAX_FRONT 192  /* largest front, in unknowns: the packed front of t + 192 rows fills the 160 KiB LDS of a CU */
#define HOMMX_MESH_FLAG_TREE 1    /* hommx_mesh_desc.flags: take the tree route whatever the frontal width                   */
#define HOMMX_MESH_FLAG_LOADS 2   /* hommx_mesh_desc.flags: a plan of the frontal route gets a load solve ("mesh_front_subst": the
                                   * response outputs of hommx_loads_source, hommx_second_sensitivity_source); without it such a plan
                                   * refuses them.  Ignored on the tree route, which has its own; the plan's descriptor keeps the bit */
/* hommx_mesh_desc.flags, value 4: a plan of the tree route does its load solves by substitution on the kept fronts of the chunk's canonical
 * pass ("mesh_multifrontal_subst") instead of a second elimination; accepted and without effect on the frontal route.  Off by default */
#define HOMMX_MESH_FLAG_TREE_LOADS HOMMX_FLAG_TREE_LOADS

typedef struct hommx_mesh_desc {
  int32_t dim, kind, device, flags;   /* as hommx_plan_desc; flags: 0 or HOMMX_MESH_FLAG_* or'ed                  */
  int64_t n_nodes;                    /* independent (periodic) nodes                                             */
  int64_t n_el;                       /* micro elements; coef[cell][el] follows THIS order                        */
  const int32_t* el_nodes;            /* [n_el][dim+1]  periodic node of each vertex                              */
  const double* el_x;                 /* [n_el][dim+1][dim] vertex coordinates, NOT folded: gradients and volumes */
  const int32_t* order;               /* [n_nodes] elimination order, or NULL: the library's own (narrowest of reverse Cuthill-McKee and coordinate sweeps); the tree route checks it and ignores it */
  int32_t reserved[4];
} hommx_mesh_desc;

/* Validation and symbolic phase only, no GPU: node range, every node used, no repeated node in an element, non-degenerate elements,
 * element volumes summing to 1 (the unit cell), a connected mesh, `order` a permutation, front width <= HOMMX_MESH_MAX_FRONT.  Any
 * failure returns HOMMX_EINVAL with the reason (the measured width and the limit for a front that is too wide).  Either output may
 * be NULL. */
int hommx_mesh_analyze(const hommx_mesh_desc* d, int32_t* front_width, double* flops_per_solve);
/* The tree route's analysis, host only: the same checks but the front width, then the dissection.  Supernodes (fronts) are numbered in
 * elimination order, children before their parent, the root last; parent[root] = -1, no front has more than two children, and the gauge
 * is the root's node of highest id.  max_front: the largest front (eliminated + boundary unknowns); flops_per_solve: the multifrontal
 * model.  A node with more than 127 coupling codes (neighbours + itself) is refused with HOMMX_EINVAL.  Every output may be NULL;
 * parent needs n_fronts entries (a first call without it tells how many). */
int hommx_mesh_analyze_tree(const hommx_mesh_desc* d, int32_t* n_fronts, int32_t* n_groups, int32_t* max_front, double* flops_per_solve,
                            int32_t* supernode_of_node /*[n_nodes] or NULL*/, int32_t* parent /*[n_fronts] or NULL*/);
/* The same checks, then the plan on d->device: the frontal route when its width is at most HOMMX_MESH_MAX_FRONT and the flag is not
 * set, the tree route otherwise (a front too wide is then no error). */
int hommx_plan_create_mesh(hommx_plan** out, const hommx_mesh_desc* d);
/* Front width of a frontal mesh plan in unknowns; 0 for the structured routes and for the tree route. */
int32_t hommx_plan_front_width(const hommx_plan* plan);

/*
 * Multi-GPU from ONE process: the macro cells are block-partitioned over the devices of a communicator --
 * the reference's MPI partition of the cell loop (hmm.py:307-310) -- and ONE RCCL all-gather over xGMI returns the whole
 * effective-tensor field (with the per-cell info flags riding in the same buffer) to every device, where the reference merges
 * rank contributions in PETSc's assembly stash (hmm.py:325-330, :442).  RCCL is loaded lazily (dlopen) on the first call.
 * Python callers that run one process per GPU use hommx_amd/dist.py instead.
 *
 *   hommx_comm_init_all     communicator over devs[0..ndev) (NULL: devices 0..ndev-1); one stream per device
 *   hommx_allgather_field   in-place all-gather: d_field_per_dev[i] is a device buffer of ndev * count doubles on device i whose
 *                           own shard already sits at offset i * count; returns after every device holds all shards
 *   hommx_solve_batch_multi plans[i] = a plan created on device i of the communicator (same dim / n_micro / kind); host
 *                           pointers as hommx_solve_batch.  Device i receives, solves and packs ONLY cells
 *                           [i * ceil(n/ndev), (i+1) * ceil(n/ndev)); the field is all-gathered and copied out once.
 */
typedef struct hommx_comm hommx_comm;
int hommx_comm_init_all(hommx_comm** out, int ndev, const int* devs);
int hommx_comm_destroy(hommx_comm* comm);
int hommx_comm_size(const hommx_comm* comm);
int hommx_allgather_field(hommx_comm* comm, double* const* d_field_per_dev, int64_t count_per_dev);
int hommx_solve_batch_multi(hommx_comm* comm, hommx_plan* const* plans, int64_t n_cells, const double* coef, const double* M,
                            double* A_eff, int32_t* info);

/* DEVICE-pointer form: the inputs stay resident on their devices (no H2D per call).  d_coef_per_dev[i] / d_M_per_dev[i] point at
 * the shard of device i (cells [begin_i, end_i) of hommx_shard_range, its own first cell at offset 0) on device i;
 * d_packed_per_dev[i] is a buffer of ndev * per_dev * (t*t + 1) doubles on device i that receives the whole gathered field, one row
 * [A_eff (t*t) | info as a double] per cell slot, shard after (padded) shard -- hommx_unpack_field() reads that layout on the host.
 * Returns after the all-gather has completed on every device. */
int hommx_solve_batch_multi_device(hommx_comm* comm, hommx_plan* const* plans, int64_t n_cells, const double* const* d_coef_per_dev,
                                   const double* const* d_M_per_dev, double* const* d_packed_per_dev);

/* The block partition and the layout of the gathered field as plain host arithmetic (no GPU needed): cells of device i are
 * [begin, end) = [i * per_dev, min(n_cells, (i+1) * per_dev)), per_dev = ceil(n_cells / ndev)  (the reference's
 * MPI ownership ranges, hmm.py:307-310). */
int hommx_shard_range(int64_t n_cells, int32_t ndev, int32_t i, int64_t* begin, int64_t* end, int64_t* per_dev);
int hommx_unpack_field(int64_t n_cells, int32_t ndev, int32_t tt, const double* packed, double* A_eff, int32_t* info);

/* Calibration micro-benchmark, in FLOP/s: the best sustained rate of v_mfma_f64_16x16x4_f64 (8 independent accumulator tiles per
 * wave) and of v_fma_f64 (16 independent accumulators per lane) over 2 and 4 waves per SIMD on all CUs.  Both instructions share one
 * fp64 pipe on MI355X; bench.py reports the larger as the measured fp64 peak next to the datasheet figure.
 * hommx_calibrate_fp64_mfma is the MFMA figure alone (kept for callers of the first ABI revision). */
int hommx_calibrate_fp64(int device, double* mfma_flops_per_s, double* fma_flops_per_s);
int hommx_calibrate_fp64_mfma(int device, double* flops_per_s);
/* Same plus a third figure: the MFMA fed from LDS the way the GEMM kernels feed it (16 MFMAs per 16 ds_read_b64).  The dependency-free
 * pure-MFMA loop clocks down under its own load; this loop is the fp64 matrix rate a real kernel can hold.  Any pointer may be NULL. */
int hommx_calibrate_fp64_detail(int device, double* mfma_flops_per_s, double* fma_flops_per_s, double* mfma_lds_fed_flops_per_s);

const char* hommx_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HOMMX_HIP_H */
