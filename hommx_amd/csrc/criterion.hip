// criterion.hip -- failure criteria evaluated on the reconstructed micro state.
//
// For macro cell c with macro gradient / strain xi, its canonical correctors chi_m and, with a load P, the corrector chi_P of the load:
//   X    = sum_m xi_m chi_m (+ chi_P)                                         one pass over the correctors, into LDS or the cell's slot
//   e_K  = xi + sum_a sum_alpha X[p_a bs + alpha] strain(g_a, M, alpha)       gradient / strain of micro element K (shear doubled)
//   q_K  = material(coef_K) e_K (+ P_K)                                       flux / stress (shear not doubled): k_recon's element<>()
//   v_K  = program(x, f, e_K, q_K, coef_K, y_K)                               the criterion: ONE scalar, interpreted once per element
// and the statistics  max_K v_K  with the smallest element reaching it (a NaN never wins),  sum |K| v_K  (a NaN makes it NaN) and
// sum |K| [v_K >= threshold].  OUT also writes v_K and / or e_K, q_K: the totals the program saw.
//
// One workgroup of kWalkThreads per macro cell on the pieces of elem_walk.h; the reductions are its fixed-order ones, so a cell's
// statistics do not depend on its batch position, the chunking or on OUT.  The whole kernel body is compiled without contraction: which
// products would fuse into an fma depends on the instantiation (with OUT the strain and the flux have one more use), and what the
// program sees must not.
//
// The interpreter is the value pass of coef_program.hip's, on one element instead of a quadrature loop: the program travels by value in
// the arguments, the dispatch is a scalar branch on readfirstlane of the opcode, every operation one separately rounded IEEE operation
// in program order (hommx_amd.expr.Criterion.host_values is its NumPy twin).  The top of the stack is a register; the levels below it
// are rows of dynamic LDS, stack[depth - 1][kWalkThreads], lane-contiguous (no bank conflict; a thread touches its own column only: no
// barrier), sized at launch from the program's validated depth.  The inputs: x and the 2 t state values are selected by switches on the
// uniform operand over static registers (no register array is indexed dynamically, hence no scratch); a field f[k], y[i] (the element
// centroid) and c[k] are vector loads where they are read -- the cell's row, the shared centroids and the element's own coefficient
// entry stay in cache, and the 21 Voigt entries are not held live.  No atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include "coef_program.h"
#include "elem_walk.h"
#include "kernels.h"

namespace hommx {

namespace {

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// a[j], j uniform and below T: a switch over the static registers
template <int T>
__device__ __forceinline__ double pick(int j, const double (&a)[T]) {
  double v = a[0];
  switch (j) {
    case 1:
      if constexpr (T > 1) v = a[1];
      break;
    case 2:
      if constexpr (T > 2) v = a[2];
      break;
    case 3:
      if constexpr (T > 3) v = a[3];
      break;
    case 4:
      if constexpr (T > 4) v = a[4];
      break;
    case 5:
      if constexpr (T > 5) v = a[5];
      break;
    default: break;
  }
  return v;
}

// The criterion of one element.  x: the midpoint; row: the cell's row (the fields behind the midpoint); e, s: strain and flux; ce: the
// element's coefficient entry; yk: its centroid (read by Y only); stk: this thread's column of the stack rows
template <int T>
__device__ __forceinline__ double run_program(const CritArgs& A, const double (&x)[3], const double* __restrict__ row, const double (&e)[T],
                                              const double (&s)[T], const double* __restrict__ ce, const double* __restrict__ yk,
                                              double* __restrict__ stk) {
#pragma clang fp contract(off)
  const int n_ops = A.prog.n_ops, base = program_row_doubles(A.n_fields);
  double t = 0.0, result = 0.0;
  int sp = 0;  // depth: the top is t, the levels below it stk[0 .. sp-2]
  auto push = [&] {
    if (sp > 0) stk[(sp - 1) * kWalkThreads] = t;
    ++sp;
  };
  auto pop = [&]() -> double {
    --sp;
    return stk[(sp - 1) * kWalkThreads];
  };
  for (int pc = 0; pc < n_ops; ++pc) {
    const uint32_t word = A.prog.code[pc >> 1] >> ((pc & 1) * 16);  // little endian: opcode in the low byte, operand above it
    const int op = uniform(word & 0xff), k = uniform((word >> 8) & 0xff);
    switch (op) {
      case OP_CONST:
        push();
        t = A.prog.consts[k];
        break;
      case OP_X:
        push();
        if (k < 3)
          t = pick<3>(k, x);
        else if (k < base)
          t = row[k];
        else if (k < base + T)
          t = pick<T>(k - base, e);
        else if (k < base + 2 * T)
          t = pick<T>(k - base - T, s);
        else
          t = ce[k - base - 2 * T];
        break;
      case OP_Y:
        push();
        t = yk[k];
        break;
      case OP_DUP: push(); break;
      case OP_ADD: t = add_rn(pop(), t); break;
      case OP_SUB: t = add_rn(pop(), -t); break;
      case OP_MUL: t = mul_rn(pop(), t); break;
      case OP_DIV: t = div_rn(pop(), t); break;
      case OP_NEG: t = -t; break;
      case OP_ABS: t = __builtin_fabs(t); break;
      case OP_MIN: {
        const double a = pop();
        t = t < a ? t : a;
        break;
      }
      case OP_MAX: {
        const double a = pop();
        t = t > a ? t : a;
        break;
      }
      case OP_LT: t = pop() < t ? 1.0 : 0.0; break;
      case OP_LE: t = pop() <= t ? 1.0 : 0.0; break;
      case OP_GT: t = pop() > t ? 1.0 : 0.0; break;
      case OP_GE: t = pop() >= t ? 1.0 : 0.0; break;
      case OP_AND: {
        const double a = pop();
        t = (a != 0.0 && t != 0.0) ? 1.0 : 0.0;
        break;
      }
      case OP_OR: {
        const double a = pop();
        t = (a != 0.0 || t != 0.0) ? 1.0 : 0.0;
        break;
      }
      case OP_NOT: t = t == 0.0 ? 1.0 : 0.0; break;
      case OP_SELECT: {
        const double a = pop(), c = pop();
        t = c != 0.0 ? a : t;
        break;
      }
      case OP_SQRT: t = ::sqrt(t); break;
      case OP_SIN: t = ::sin(t); break;
      case OP_COS: t = ::cos(t); break;
      case OP_TAN: t = ::tan(t); break;
      case OP_EXP: t = ::exp(t); break;
      case OP_LOG: t = ::log(t); break;
      case OP_TANH: t = ::tanh(t); break;
      default:  // OP_STORE 0: the validation admits no other opcode, and one component
        result = t;
        --sp;
        if (sp > 0) t = stk[(sp - 1) * kWalkThreads];
        break;
    }
  }
  return result;
}

template <int DIM, int KIND, bool MESH, bool OUT>
__global__ __launch_bounds__(kWalkThreads) void k_criterion(CritArgs A) {
#pragma clang fp contract(off)
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, BS = ks.bs, NCOMP = ks.n_comp;
  extern __shared__ double lds_dyn[];  // [the field (ndof), unless it lies in the slot | stack[depth - 1][kWalkThreads]]
  __shared__ double red[kWalkWaves][2], red_max[kWalkWaves][2];
  const int tid = threadIdx.x;
  const long long cell = blockIdx.x;
  const long long ndof = A.ndof;

  double xi[T];
#pragma unroll
  for (int m = 0; m < T; ++m) xi[m] = A.xi[cell * T + m];
  double Mp[DIM * DIM];
  cell_M<DIM>(A.M, cell, Mp);
  const double* row = A.rows + cell * program_row_doubles(A.n_fields);
  const double x[3] = {row[0], row[1], row[2]};

  // X = sum_m xi_m chi_m (+ chi_P): every corrector of the cell read once, lanes along the dof index
  double* X = A.slot ? A.slot + cell * ndof : lds_dyn;
  double* stk = (A.slot ? lds_dyn : lds_dyn + ndof) + tid;
  const double* corr = A.corr + cell * T * ndof;
  const double* chi_P = A.corr_load ? A.corr_load + cell * T * ndof : nullptr;
  for (long long j = tid; j < ndof; j += kWalkThreads) {
    double v = 0.0;
#pragma unroll
    for (int m = 0; m < T; ++m) v += xi[m] * corr[m * ndof + j];
    if (chi_P) v += chi_P[j];
    X[j] = v;
  }
  __syncthreads();

  const double* cc = A.coef + cell * A.n_el * NCOMP;
  const double* P = A.P ? A.P + (A.per_cell ? cell : 0) * A.n_el * T : nullptr;
  double mx = -__builtin_inf(), sum_v = 0.0, sum_over = 0.0;
  long long arg = -1;
  for_elements<DIM, MESH>(A, tid, [&](long long el, double vol, auto vertex) {
#pragma clang fp contract(off)
    double e[T];
#pragma unroll
    for (int m = 0; m < T; ++m) e[m] = xi[m];
#pragma unroll
    for (int a = 0; a < DIM + 1; ++a) {
      int node;
      double g[DIM];
      vertex(a, node, g);
#pragma unroll
      for (int al = 0; al < BS; ++al) {
        const double c = X[(long long)node * BS + al];
        double sa[T];
        strain<DIM, KIND>(g, Mp, al, sa);
#pragma unroll
        for (int m = 0; m < T; ++m) e[m] += c * sa[m];
      }
    }
    const double* __restrict__ ce = cc + el * NCOMP;
    double q[T];
    {
      double C[T][T];
      material<DIM, KIND>(ce, C);
#pragma unroll
      for (int m = 0; m < T; ++m) {
        double v = 0.0;
#pragma unroll
        for (int n = 0; n < T; ++n) v += C[m][n] * e[n];
        q[m] = P ? v + P[el * T + m] : v;
      }
    }
    const double v = run_program<T>(A, x, row, e, q, ce, A.points + el * DIM, stk);
    if constexpr (OUT) {
      if (A.values) A.values[cell * A.n_el + el] = v;
      if (A.strain) {
        double* __restrict__ srow = A.strain + (cell * A.n_el + el) * T;
        double* __restrict__ qrow = A.flux + (cell * A.n_el + el) * T;
#pragma unroll
        for (int m = 0; m < T; ++m) {
          srow[m] = e[m];
          qrow[m] = q[m];
        }
      }
    }
    sum_v += vol * v;
    sum_over += v >= A.threshold ? vol : 0.0;
    if (v > mx) {
      mx = v;
      arg = el;
    }
  });

  double barg = (double)arg;
  block_argmax(mx, barg, red_max, tid);
  double sums[2] = {sum_v, sum_over};
  double* out = A.crit + cell * 4;
  block_sums<2>(sums, red, tid, [&](int q, double total) { out[2 + q] = total; });
  if (tid == 0) {
    out[0] = mx;
    out[1] = barg;
  }
}

}  // namespace

size_t criterion_lds_bytes(long long ndof, int depth) { return sizeof(double) * ((size_t)ndof + (size_t)kWalkThreads * (depth - 1)); }

hipError_t launch_criterion(const CritArgs& a, int depth, long long nc, hipStream_t st) {
  if (nc <= 0) return hipSuccess;
  if (depth < 1 || depth > PROGRAM_MAX_STACK || a.prog.n_comp != 1) return hipErrorInvalidValue;
  const auto kernel = a.values || a.strain ? walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_criterion<D(), K(), MESH(), true>; })
                                           : walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_criterion<D(), K(), MESH(), false>; });
  const size_t lds = criterion_lds_bytes(a.slot ? 0 : a.ndof, depth);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  return launch_walk(a, nc, st, kernel, lds);
}

}  // namespace hommx
