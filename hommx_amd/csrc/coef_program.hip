// coef_program.hip -- expression coefficients sampled on the device: a bytecode interpreter expands the program of a
// HOMMX_COEF_PROGRAM source (include/hommx_hip.h; coef_program.h) into the plan's element stream.
//
// One thread per (cell, element), 256 per block.  The program travels by value in the kernel arguments and is the same for every
// thread, so the dispatch is a scalar branch on readfirstlane of the opcode: no divergence, whatever the program.  The top of the value
// stack lives in a register, the rest in LDS as stack[depth][thread] -- consecutive lanes on consecutive 8-byte words, so no access has
// a bank conflict, and a thread only ever touches its own column, so there is no barrier.  32 KiB per block; 140 VGPRs: 3 waves/SIMD.  No
// register array is indexed dynamically (x, y and the component accumulators are selected by switches on the uniform operand), hence no
// scratch.  Every arithmetic operation is one separately rounded IEEE operation (no contraction), in the order of the program, so a host
// that interprets the same program (hommx_amd.expr.Expression.host_stream) reproduces the stream bit for bit wherever the program
// contains exactly rounded operations only.
#include "coef_program.h"

#include "kernels.h"

namespace hommx {

namespace {

constexpr int BLOCK = 256;

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ double pick3(int k, double a0, double a1, double a2) { return k == 0 ? a0 : k == 1 ? a1 : a2; }

__global__ __launch_bounds__(BLOCK) void k_expand_program(const ProgramArgs prog, const double* __restrict__ points,
                                                         const double* __restrict__ weights, int n_q, int dim,
                                                         const double* __restrict__ mid, double* __restrict__ coef, long long n_el,
                                                         long long total) {
#pragma clang fp contract(off)
  __shared__ double stack[PROGRAM_MAX_STACK][BLOCK];
  const int tid = threadIdx.x;
  const long long idx = (long long)blockIdx.x * BLOCK + tid;
  if (idx >= total) return;  // the tail of the grid; nothing below synchronises
  const long long cell = idx / n_el, el = idx - cell * n_el;
  const double x0 = mid[cell * 3], x1 = mid[cell * 3 + 1], x2 = mid[cell * 3 + 2];
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
          t = pick3(k, x0, x1, x2);
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

}  // namespace

hipError_t launch_expand_program(const ProgramArgs& prog, const double* d_points, const double* d_weights, int n_q, int dim,
                                 const double* d_mid, double* d_coef, long long n_el, long long ncells, hipStream_t stream) {
  const long long total = ncells * n_el;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_expand_program, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, prog, d_points, d_weights,
                     n_q, dim, d_mid, d_coef, n_el, total);
  return hipGetLastError();
}

}  // namespace hommx
