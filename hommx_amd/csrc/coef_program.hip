// coef_program.hip -- expression coefficients sampled on the device: a bytecode interpreter expands the program of a
// HOMMX_COEF_PROGRAM source (include/hommx_hip.h; coef_program.h) into the plan's element stream.
//
// One thread per (cell, element), 256 per block.  The program travels by value in the kernel arguments and is the same for every
// thread, so the dispatch is a scalar branch on readfirstlane of the opcode: no divergence, whatever the program.  The top of the value
// stack lives in a register, the rest in LDS as stack[depth][thread] -- consecutive lanes on consecutive 8-byte words, so no access has
// a bank conflict, and a thread only ever touches its own column, so there is no barrier.  32 KiB per block; 142 VGPRs: 3 waves/SIMD.  No
// register array is indexed dynamically (x, y and the component accumulators are selected by switches on the uniform operand), hence no
// scratch.  Every arithmetic operation is one separately rounded IEEE operation (no contraction), in the order of the program, so a host
// that interprets the same program (hommx_amd.expr.Expression.host_stream) reproduces the stream bit for bit wherever the program
// contains exactly rounded operations only.
//
// The per-cell row is the midpoint and then the n_fields fields of the cell (coef_program.h, program_row_doubles).  The midpoint lives in
// registers; a field does not -- `X k`, k >= 3, loads row[k] where it is read.  The row is 32 .. 56 bytes and stays in cache, the lanes
// of a wave may belong to different cells (a vector load, not a scalar one), and the forward-mode kernel of four slots has no
// registers to spare for four more live doubles.  A program without fields never takes that branch and computes what it always did.
#include "coef_program.h"

#include "kernels.h"

namespace hommx {

namespace {

constexpr int BLOCK = 256;

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ double pick3(int k, double a0, double a1, double a2) { return k == 0 ? a0 : k == 1 ? a1 : a2; }

__global__ __launch_bounds__(BLOCK) void k_expand_program(const ProgramArgs prog, const double* __restrict__ points,
                                                         const double* __restrict__ weights, int n_q, int dim,
                                                         const double* __restrict__ mid, int n_fields, double* __restrict__ coef,
                                                         long long n_el, long long total) {
#pragma clang fp contract(off)
  __shared__ double stack[PROGRAM_MAX_STACK][BLOCK];
  const int tid = threadIdx.x;
  const long long idx = (long long)blockIdx.x * BLOCK + tid;
  if (idx >= total) return;  // the tail of the grid; nothing below synchronises
  const long long cell = idx / n_el, el = idx - cell * n_el;
  const double* row = mid + cell * program_row_doubles(n_fields);  // the midpoint, then the fields of the cell
  const double x0 = row[0], x1 = row[1], x2 = row[2];
  const double* yp = points + el * n_q * dim;
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0, acc4 = 0.0, acc5 = 0.0;
  const int n_ops = prog.n_ops;
  for (int q = 0; q < n_q; ++q) {
    const double y0 = yp[q * dim], y1 = yp[q * dim + 1], y2 = dim > 2 ? yp[q * dim + 2] : 0.0;
    const double w = weights[q];
    // depth sp: the top is `t`, the values below it stack[1 .. sp-1][tid] (a push at depth 0 parks the dead `t` in row 0)
    double t = 0.0;
    int sp = 0;
    for (int pc = 0; pc < n_ops; ++pc) {
      const uint32_t word = prog.code[pc >> 1] >> ((pc & 1) * 16);  // little endian: opcode in the low byte, operand above it
      const int op = uniform(word & 0xff), k = uniform((word >> 8) & 0xff);
      switch (op) {
        case OP_CONST:
          stack[sp++][tid] = t;
          t = prog.consts[k];
          break;
        case OP_X:
          stack[sp++][tid] = t;
          t = k < 3 ? pick3(k, x0, x1, x2) : row[k];  // a field: loaded where it is read (uniform k: a scalar branch, a vector load)
          break;
        case OP_Y:
          stack[sp++][tid] = t;
          t = pick3(k, y0, y1, y2);
          break;
        case OP_DUP: stack[sp++][tid] = t; break;
        case OP_ADD: t = add_rn(stack[--sp][tid], t); break;
        case OP_SUB: t = add_rn(stack[--sp][tid], -t); break;
        case OP_MUL: t = mul_rn(stack[--sp][tid], t); break;
        case OP_DIV: t = div_rn(stack[--sp][tid], t); break;
        case OP_NEG: t = -t; break;
        case OP_ABS: t = __builtin_fabs(t); break;
        case OP_MIN: {
          const double a = stack[--sp][tid];
          t = t < a ? t : a;
          break;
        }
        case OP_MAX: {
          const double a = stack[--sp][tid];
          t = t > a ? t : a;
          break;
        }
        case OP_LT: t = stack[--sp][tid] < t ? 1.0 : 0.0; break;
        case OP_LE: t = stack[--sp][tid] <= t ? 1.0 : 0.0; break;
        case OP_GT: t = stack[--sp][tid] > t ? 1.0 : 0.0; break;
        case OP_GE: t = stack[--sp][tid] >= t ? 1.0 : 0.0; break;
        case OP_AND: {
          const double a = stack[--sp][tid];
          t = (a != 0.0 && t != 0.0) ? 1.0 : 0.0;
          break;
        }
        case OP_OR: {
          const double a = stack[--sp][tid];
          t = (a != 0.0 || t != 0.0) ? 1.0 : 0.0;
          break;
        }
        case OP_NOT: t = t == 0.0 ? 1.0 : 0.0; break;
        case OP_SELECT: {
          const double a = stack[--sp][tid], c = stack[--sp][tid];
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
        default: {  // OP_STORE: the validation admits no other opcode
          const double v = mul_rn(w, t);
          switch (k) {
            case 0: acc0 = add_rn(acc0, v); break;
            case 1: acc1 = add_rn(acc1, v); break;
            case 2: acc2 = add_rn(acc2, v); break;
            case 3: acc3 = add_rn(acc3, v); break;
            case 4: acc4 = add_rn(acc4, v); break;
            default: acc5 = add_rn(acc5, v); break;
          }
          t = stack[--sp][tid];
          break;
        }
      }
    }
  }
  double* out = coef + idx * prog.n_comp;
  out[0] = acc0;
  if (prog.n_comp > 1) out[1] = acc1;
  if (prog.n_comp > 2) out[2] = acc2;
  if (prog.n_comp > 3) out[3] = acc3;
  if (prog.n_comp > 4) out[4] = acc4;
  if (prog.n_comp > 5) out[5] = acc5;
}

// -- forward mode: the stream and its derivatives with respect to the parameters (the first n_params constants) and the fields ----------
// The differentiable slots are the parameters, then the fields (n_tan = n_params + n_fields <= P): `X k`, k >= 3, seeds slot
// n_params + k - 3 as `CONST k`, k < n_params, seeds slot k.
// The rules of include/hommx_hip.h (hommx_expand_tangents), which hommx_amd.expr._run_tangent restates with NumPy.  A stack entry is
// (v, d_0 .. d_{P-1}); the value part is computed by exactly the operations of k_expand_program, so the value stream is that kernel's bit
// for bit.  Where every operand's d_j is 0.0 the result's d_j is +0.0 and the formula does not count (live1 / live2 below): a sqrt(0) or
// a division by zero in a part of the expression that does not read p[j] cannot make its tangent NaN -- and the cosine of SIN (the sine
// of COS) is not evaluated at all by a wave none of whose lanes carries a tangent through the call.
//
// Same shape as k_expand_program: one thread per (cell, element), the program by value, a scalar branch per instruction, the top of the
// stack in registers (1 + P doubles), the rest in LDS as stack[depth][1 + P][thread] -- consecutive lanes on consecutive 8-byte words,
// no bank conflict, no barrier.  Static LDS is 16 (1 + P) BLOCK 8 bytes, so the block shrinks with P: 128 threads for P = 1 (32 KiB)
// and P = 2 (48 KiB), one wave of 64 for P = 4 (40 KiB); of the 160 KiB of a CU that is 5, 3 and 4 blocks.  P is a template parameter
// and every loop over j unrolls, the accumulators are selected by comparing the uniform operand with each constant index: no register
// array is indexed dynamically, hence no scratch (tests/test_expr_tangent_resources.py reads it off the code object).
constexpr int tangent_block(int P) { return P == 4 ? 64 : 128; }

template <int P>
__global__ __launch_bounds__(tangent_block(P)) void k_expand_program_tangent(const ProgramArgs prog, int n_params, int n_fields,
                                                                             const double* __restrict__ points,
                                                                             const double* __restrict__ weights, int n_q, int dim,
                                                                             const double* __restrict__ mid, double* __restrict__ coef,
                                                                             double* __restrict__ dirs, long long n_el, long long total) {
#pragma clang fp contract(off)
  constexpr int BLK = tangent_block(P);
  __shared__ double stack[PROGRAM_MAX_STACK][1 + P][BLK];
  const int tid = threadIdx.x;
  const long long idx = (long long)blockIdx.x * BLK + tid;
  if (idx >= total) return;  // the tail of the grid; nothing below synchronises
  const long long cell = idx / n_el, el = idx - cell * n_el;
  const double* row = mid + cell * program_row_doubles(n_fields);  // the midpoint, then the fields of the cell
  const double x0 = row[0], x1 = row[1], x2 = row[2];
  const int n_tan = n_params + n_fields;  // the differentiable slots: the parameters, then the fields
  const double* yp = points + el * n_q * dim;
  double acc[PROGRAM_MAX_COMP], accd[PROGRAM_MAX_COMP][P];
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
    double t = 0.0, d[P], da[P];
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
    auto flat = [&] {  // piecewise constant results
#pragma unroll
      for (int j = 0; j < P; ++j) d[j] = 0.0;
    };
    auto live1 = [&](int j) { return d[j] != 0.0; };
    auto live2 = [&](int j) { return da[j] != 0.0 || d[j] != 0.0; };
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
          t = add_rn(a, t);
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = live2(j) ? add_rn(da[j], d[j]) : 0.0;
          break;
        }
        case OP_SUB: {
          const double a = pop();
          t = add_rn(a, -t);
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = live2(j) ? add_rn(da[j], -d[j]) : 0.0;
          break;
        }
        case OP_MUL: {
          const double a = pop();
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = live2(j) ? add_rn(mul_rn(a, d[j]), mul_rn(da[j], t)) : 0.0;
          t = mul_rn(a, t);
          break;
        }
        case OP_DIV: {
          const double a = pop(), v = div_rn(a, t);
#pragma unroll
          for (int j = 0; j < P; ++j) {
            double r = 0.0;
            if (live2(j)) r = div_rn(add_rn(da[j], -mul_rn(v, d[j])), t);
            d[j] = r;
          }
          t = v;
          break;
        }
        case OP_NEG:
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = live1(j) ? -d[j] : 0.0;
          t = -t;
          break;
        case OP_ABS:
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = live1(j) ? (t < 0.0 ? -d[j] : d[j]) : 0.0;
          t = __builtin_fabs(t);
          break;
        case OP_MIN: {
          const double a = pop();
          const bool top = t < a;
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = live2(j) ? (top ? d[j] : da[j]) : 0.0;
          t = top ? t : a;
          break;
        }
        case OP_MAX: {
          const double a = pop();
          const bool top = t > a;
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = live2(j) ? (top ? d[j] : da[j]) : 0.0;
          t = top ? t : a;
          break;
        }
        case OP_LT: t = stack[--sp][0][tid] < t ? 1.0 : 0.0; flat(); break;
        case OP_LE: t = stack[--sp][0][tid] <= t ? 1.0 : 0.0; flat(); break;
        case OP_GT: t = stack[--sp][0][tid] > t ? 1.0 : 0.0; flat(); break;
        case OP_GE: t = stack[--sp][0][tid] >= t ? 1.0 : 0.0; flat(); break;
        case OP_AND: {
          const double a = stack[--sp][0][tid];
          t = (a != 0.0 && t != 0.0) ? 1.0 : 0.0;
          flat();
          break;
        }
        case OP_OR: {
          const double a = stack[--sp][0][tid];
          t = (a != 0.0 || t != 0.0) ? 1.0 : 0.0;
          flat();
          break;
        }
        case OP_NOT: t = t == 0.0 ? 1.0 : 0.0; flat(); break;
        case OP_SELECT: {
          const double a = pop(), c = stack[--sp][0][tid];  // a condition carries no tangent
          const bool first = c != 0.0;
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = live2(j) ? (first ? da[j] : d[j]) : 0.0;
          t = first ? a : t;
          break;
        }
        case OP_SQRT:
          t = ::sqrt(t);
#pragma unroll
          for (int j = 0; j < P; ++j) {
            double r = 0.0;
            if (live1(j)) r = div_rn(d[j], mul_rn(2.0, t));
            d[j] = r;
          }
          break;
        case OP_SIN: {
          bool any = false;
#pragma unroll
          for (int j = 0; j < P; ++j) any = any || live1(j);
          double c = 0.0;
          if (any) c = ::cos(t);
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = live1(j) ? mul_rn(c, d[j]) : 0.0;
          t = ::sin(t);
          break;
        }
        case OP_COS: {
          bool any = false;
#pragma unroll
          for (int j = 0; j < P; ++j) any = any || live1(j);
          double s = 0.0;
          if (any) s = ::sin(t);
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = live1(j) ? -mul_rn(s, d[j]) : 0.0;
          t = ::cos(t);
          break;
        }
        case OP_TAN: {
          t = ::tan(t);
          const double g = add_rn(1.0, mul_rn(t, t));
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = live1(j) ? mul_rn(d[j], g) : 0.0;
          break;
        }
        case OP_EXP:
          t = ::exp(t);
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = live1(j) ? mul_rn(t, d[j]) : 0.0;
          break;
        case OP_LOG:
#pragma unroll
          for (int j = 0; j < P; ++j) {
            double r = 0.0;
            if (live1(j)) r = div_rn(d[j], t);
            d[j] = r;
          }
          t = ::log(t);
          break;
        case OP_TANH: {
          t = ::tanh(t);
          const double g = add_rn(1.0, -mul_rn(t, t));
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = live1(j) ? mul_rn(d[j], g) : 0.0;
          break;
        }
        default: {  // OP_STORE: the validation admits no other opcode
          const double v = mul_rn(w, t);
#pragma unroll
          for (int c = 0; c < PROGRAM_MAX_COMP; ++c)
            if (k == c) {  // uniform: a scalar branch, and every index a constant
              acc[c] = add_rn(acc[c], v);
#pragma unroll
              for (int j = 0; j < P; ++j) accd[c][j] = add_rn(accd[c][j], mul_rn(w, d[j]));
            }
          --sp;
          t = stack[sp][0][tid];
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = stack[sp][1 + j][tid];
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

hipError_t launch_expand_program_tangent(const ProgramArgs& prog, int n_params, int n_fields, const double* d_points,
                                         const double* d_weights, int n_q, int dim, const double* d_mid, double* d_coef, double* d_dirs,
                                         long long n_el, long long ncells, hipStream_t stream) {
  const long long total = ncells * n_el;
  if (total <= 0) return hipSuccess;
  auto launch = [&](auto kernel, int block) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + block - 1) / block)), dim3(block), 0, stream, prog, n_params, n_fields, d_points,
                       d_weights, n_q, dim, d_mid, d_coef, d_dirs, n_el, total);
  };
  const int n_tan = n_params + n_fields;
  if (n_tan == 1)
    launch(k_expand_program_tangent<1>, tangent_block(1));
  else if (n_tan == 2)
    launch(k_expand_program_tangent<2>, tangent_block(2));
  else  // 3 slots run the kernel of 4 with a tangent nothing seeds and nothing stores
    launch(k_expand_program_tangent<4>, tangent_block(4));
  return hipGetLastError();
}

hipError_t launch_expand_program(const ProgramArgs& prog, const double* d_points, const double* d_weights, int n_q, int dim,
                                 const double* d_mid, int n_fields, double* d_coef, long long n_el, long long ncells,
                                 hipStream_t stream) {
  const long long total = ncells * n_el;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_expand_program, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, prog, d_points, d_weights,
                     n_q, dim, d_mid, n_fields, d_coef, n_el, total);
  return hipGetLastError();
}

}  // namespace hommx
