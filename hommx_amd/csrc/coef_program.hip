// coef_program.hip -- expression coefficients sampled on the device: a bytecode interpreter expands the program of a
// HOMMX_COEF_PROGRAM source (include/hommx_hip.h; coef_program.h) into the plan's element stream and, in forward mode, into its
// derivatives with respect to the differentiable slots.
//
// ONE kernel template, k_expand_program<P>: a stack entry is (v, d_0 .. d_{P-1}), and the value pass is the instantiation without
// tangents, P = 0.  Every opcode has one case that states its value rule and its tangent rule; every loop over j is unrolled over the
// template parameter and is not there for P = 0, so one set of statements computes `t` whatever P is: the value stream of the tangent
// pass is the value pass's bit for bit by construction.
//
// One thread per (cell, element).  The program travels by value in the kernel arguments and is the same for every thread, so the
// dispatch is a scalar branch on readfirstlane of the opcode: no divergence, whatever the program.  The top of the stack lives in
// registers (1 + P doubles), the rest in LDS as stack[depth][1 + P][thread] -- consecutive lanes on consecutive 8-byte words, so no
// access has a bank conflict, and a thread only ever touches its own column, so there is no barrier.  Static LDS is 16 (1 + P) BLOCK 8
// bytes, so the block shrinks with P (program_block): 256 threads for P = 0 (32 KiB), 128 for P = 1 (32 KiB) and P = 2 (48 KiB), one
// wave of 64 for P = 4 (40 KiB); of the 160 KiB of a CU that is 5, 5, 3 and 4 blocks.  No register array is indexed dynamically (x, y
// and the accumulators are selected by switches on the uniform operand), hence no scratch
// (tests/test_expr_program_resources.py reads it off the code object; profiles/coef_program_resource_usage.txt).  Every arithmetic
// operation is one separately rounded IEEE operation (no contraction), in the order of the program, so a host that interprets the same
// program (hommx_amd.expr.Expression.host_stream / host_tangents) reproduces the streams bit for bit wherever the program contains
// exactly rounded operations only.
//
// The per-cell row is the midpoint and then the n_fields fields of the cell (coef_program.h, program_row_doubles).  The midpoint lives in
// registers; a field does not -- `X k`, k >= 3, loads row[k] where it is read.  The row is 32 .. 56 bytes and stays in cache, the lanes
// of a wave may belong to different cells (a vector load, not a scalar one), and the instantiation of four slots has no registers to
// spare for four more live doubles.  A program without fields never takes that branch.
//
// Forward mode: the differentiable slots are the parameters (the first n_params constants), then the fields (n_tan = n_params + n_fields
// <= P): `CONST k`, k < n_params, seeds slot k, and `X k`, k >= 3, seeds slot n_params + k - 3.  The rules are those of
// include/hommx_hip.h (hommx_expand_tangents), which hommx_amd.expr._run restates with NumPy.  Where every operand's d_j is 0.0 the
// result's d_j is +0.0 and the formula does not count (rule1 / rule2 below): a sqrt(0) or a division by zero in a part of the expression
// that does not read slot j cannot make its tangent NaN -- and the cosine of SIN (the sine of COS) is not evaluated at all by a wave
// none of whose lanes carries a tangent through the call, nor by the value pass.
#include "coef_program.h"

#include "kernels.h"

namespace hommx {

namespace {

constexpr int program_block(int P) { return P == 0 ? 256 : P == 4 ? 64 : 128; }

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ double pick3(int k, double a0, double a1, double a2) { return k == 0 ? a0 : k == 1 ? a1 : a2; }

template <int P>
__global__ __launch_bounds__(program_block(P)) void k_expand_program(const ProgramArgs prog, int n_params, int n_fields,
                                                                     const double* __restrict__ points,
                                                                     const double* __restrict__ weights, int n_q, int dim,
                                                                     const double* __restrict__ mid, double* __restrict__ coef,
                                                                     double* __restrict__ dirs, long long n_el, long long total) {
#pragma clang fp contract(off)
  constexpr int BLK = program_block(P), PN = P ? P : 1;  // PN: no array of length zero; what P = 0 declares with it is never touched
  __shared__ double stack[PROGRAM_MAX_STACK][1 + P][BLK];
  const int tid = threadIdx.x;
  const long long idx = (long long)blockIdx.x * BLK + tid;
  if (idx >= total) return;  // the tail of the grid; nothing below synchronises
  const long long cell = idx / n_el, el = idx - cell * n_el;
  const double* row = mid + cell * program_row_doubles(n_fields);  // the midpoint, then the fields of the cell
  const double x0 = row[0], x1 = row[1], x2 = row[2];
  const int n_tan = n_params + n_fields;  // the differentiable slots: the parameters, then the fields
  const double* yp = points + el * n_q * dim;
  double acc[PROGRAM_MAX_COMP], accd[PROGRAM_MAX_COMP][PN];
#pragma unroll
  for (int c = 0; c < PROGRAM_MAX_COMP; ++c) {
    acc[c] = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) accd[c][j] = 0.0;
  }
  const int n_ops = prog.n_ops;
  for (int q = 0; q < n_q; ++q) {
    const double y0 = yp[q * dim], y1 = yp[q * dim + 1], y2 = dim > 2 ? yp[q * dim + 2] : 0.0;
    const double w = weights[q];
    // depth sp: the top is (t, d), the entries below it stack[1 .. sp-1][.][tid] (a push at depth 0 parks the dead top in row 0)
    double t = 0.0, d[PN], da[PN];
#pragma unroll
    for (int j = 0; j < P; ++j) d[j] = 0.0;
    int sp = 0;
    auto push = [&] {
      stack[sp][0][tid] = t;
#pragma unroll
      for (int j = 0; j < P; ++j) stack[sp][1 + j][tid] = d[j];
      ++sp;
    };
    auto pop = [&]() -> double {  // the entry below the top: its value, its tangents into da
      --sp;
#pragma unroll
      for (int j = 0; j < P; ++j) da[j] = stack[sp][1 + j][tid];
      return stack[sp][0][tid];
    };
    auto pop_value = [&]() -> double { return stack[--sp][0][tid]; };  // an operand whose tangent does not count
    auto flat = [&] {  // piecewise constant results
#pragma unroll
      for (int j = 0; j < P; ++j) d[j] = 0.0;
    };
    // d_j of a result of one operand (the top) / of two (the popped entry and the top): +0.0 where every operand's d_j is 0.0 and
    // f(j) is then not evaluated, else f(j) -- `rule` of hommx_amd/expr.py
    auto rule1 = [&](auto f) {
#pragma unroll
      for (int j = 0; j < P; ++j) {
        double r = 0.0;
        if (d[j] != 0.0) r = f(j);
        d[j] = r;
      }
    };
    auto rule2 = [&](auto f) {
#pragma unroll
      for (int j = 0; j < P; ++j) {
        double r = 0.0;
        if (da[j] != 0.0 || d[j] != 0.0) r = f(j);
        d[j] = r;
      }
    };
    auto any_live = [&] {  // does this lane carry a tangent in the top?  (false for P = 0)
      bool any = false;
#pragma unroll
      for (int j = 0; j < P; ++j) any = any || d[j] != 0.0;
      return any;
    };
    for (int pc = 0; pc < n_ops; ++pc) {
      const uint32_t word = prog.code[pc >> 1] >> ((pc & 1) * 16);  // little endian: opcode in the low byte, operand above it
      const int op = uniform(word & 0xff), k = uniform((word >> 8) & 0xff);
      switch (op) {
        case OP_CONST:
          push();
          t = prog.consts[k];
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = (k == j && k < n_params) ? 1.0 : 0.0;
          break;
        case OP_X:
          push();
          if (k < 3) {
            t = pick3(k, x0, x1, x2);
            flat();
          } else {  // field k - 3, loaded where it is read (uniform k: a scalar branch, a vector load); it seeds its own slot
            t = row[k];
#pragma unroll
            for (int j = 0; j < P; ++j) d[j] = (j == n_params + k - 3) ? 1.0 : 0.0;
          }
          break;
        case OP_Y:
          push();
          t = pick3(k, y0, y1, y2);
          flat();
          break;
        case OP_DUP: push(); break;
        case OP_ADD: {
          const double a = pop();
          rule2([&](int j) { return add_rn(da[j], d[j]); });
          t = add_rn(a, t);
          break;
        }
        case OP_SUB: {
          const double a = pop();
          rule2([&](int j) { return add_rn(da[j], -d[j]); });
          t = add_rn(a, -t);
          break;
        }
        case OP_MUL: {
          const double a = pop();
          rule2([&](int j) { return add_rn(mul_rn(a, d[j]), mul_rn(da[j], t)); });
          t = mul_rn(a, t);
          break;
        }
        case OP_DIV: {
          const double a = pop(), v = div_rn(a, t);
          rule2([&](int j) { return div_rn(add_rn(da[j], -mul_rn(v, d[j])), t); });
          t = v;
          break;
        }
        case OP_NEG:
          rule1([&](int j) { return -d[j]; });
          t = -t;
          break;
        case OP_ABS:
          rule1([&](int j) { return t < 0.0 ? -d[j] : d[j]; });
          t = __builtin_fabs(t);
          break;
        case OP_MIN: {
          const double a = pop();
          const bool top = t < a;
          rule2([&](int j) { return top ? d[j] : da[j]; });
          t = top ? t : a;
          break;
        }
        case OP_MAX: {
          const double a = pop();
          const bool top = t > a;
          rule2([&](int j) { return top ? d[j] : da[j]; });
          t = top ? t : a;
          break;
        }
        case OP_LT: t = pop_value() < t ? 1.0 : 0.0; flat(); break;
        case OP_LE: t = pop_value() <= t ? 1.0 : 0.0; flat(); break;
        case OP_GT: t = pop_value() > t ? 1.0 : 0.0; flat(); break;
        case OP_GE: t = pop_value() >= t ? 1.0 : 0.0; flat(); break;
        case OP_AND: {
          const double a = pop_value();
          t = (a != 0.0 && t != 0.0) ? 1.0 : 0.0;
          flat();
          break;
        }
        case OP_OR: {
          const double a = pop_value();
          t = (a != 0.0 || t != 0.0) ? 1.0 : 0.0;
          flat();
          break;
        }
        case OP_NOT: t = t == 0.0 ? 1.0 : 0.0; flat(); break;
        case OP_SELECT: {
          const double a = pop(), c = pop_value();  // a condition carries no tangent
          const bool first = c != 0.0;
          rule2([&](int j) { return first ? da[j] : d[j]; });
          t = first ? a : t;
          break;
        }
        case OP_SQRT:
          t = ::sqrt(t);
          rule1([&](int j) { return div_rn(d[j], mul_rn(2.0, t)); });
          break;
        case OP_SIN: {
          double c = 0.0;
          if (any_live()) c = ::cos(t);
          rule1([&](int j) { return mul_rn(c, d[j]); });
          t = ::sin(t);
          break;
        }
        case OP_COS: {
          double s = 0.0;
          if (any_live()) s = ::sin(t);
          rule1([&](int j) { return -mul_rn(s, d[j]); });
          t = ::cos(t);
          break;
        }
        case OP_TAN: {
          t = ::tan(t);
          const double g = add_rn(1.0, mul_rn(t, t));
          rule1([&](int j) { return mul_rn(d[j], g); });
          break;
        }
        case OP_EXP:
          t = ::exp(t);
          rule1([&](int j) { return mul_rn(t, d[j]); });
          break;
        case OP_LOG:
          rule1([&](int j) { return div_rn(d[j], t); });
          t = ::log(t);
          break;
        case OP_TANH: {
          t = ::tanh(t);
          const double g = add_rn(1.0, -mul_rn(t, t));
          rule1([&](int j) { return mul_rn(d[j], g); });
          break;
        }
        default: {  // OP_STORE: the validation admits no other opcode
          const double v = mul_rn(w, t);
          auto add_to = [&](int c) {  // inlined with a constant c: no register array is indexed dynamically
            acc[c] = add_rn(acc[c], v);
#pragma unroll
            for (int j = 0; j < P; ++j) accd[c][j] = add_rn(accd[c][j], mul_rn(w, d[j]));
          };
          switch (k) {  // uniform: scalar branches to ONE accumulation (an unrolled `if (k == c)` becomes six additions and selects)
            case 0: add_to(0); break;
            case 1: add_to(1); break;
            case 2: add_to(2); break;
            case 3: add_to(3); break;
            case 4: add_to(4); break;
            default: add_to(5); break;
          }
          t = pop();
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = da[j];
          break;
        }
      }
    }
  }
  const int n_comp = prog.n_comp;
#pragma unroll
  for (int c = 0; c < PROGRAM_MAX_COMP; ++c)
    if (c < n_comp) {
      if (coef) coef[idx * n_comp + c] = acc[c];
#pragma unroll
      for (int j = 0; j < P; ++j)
        if (j < n_tan) dirs[((cell * n_tan + j) * n_el + el) * n_comp + c] = accd[c][j];
    }
}

}  // namespace

hipError_t launch_expand_program(const ProgramArgs& prog, int n_params, int n_fields, const double* d_points, const double* d_weights,
                                 int n_q, int dim, const double* d_rows, double* d_coef, double* d_dirs, long long n_el, long long ncells,
                                 hipStream_t stream) {
  const long long total = ncells * n_el;
  if (total <= 0) return hipSuccess;
  auto launch = [&](auto kernel, int block) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + block - 1) / block)), dim3(block), 0, stream, prog, n_params, n_fields, d_points,
                       d_weights, n_q, dim, d_rows, d_coef, d_dirs, n_el, total);
  };
  const int n_tan = n_params + n_fields;
  if (!d_dirs)  // the value pass, whatever slots the program has
    launch(k_expand_program<0>, program_block(0));
  else if (n_tan == 1)
    launch(k_expand_program<1>, program_block(1));
  else if (n_tan == 2)
    launch(k_expand_program<2>, program_block(2));
  else  // 3 slots run the kernel of 4 with a tangent nothing seeds and nothing stores
    launch(k_expand_program<4>, program_block(4));
  return hipGetLastError();
}

}  // namespace hommx
