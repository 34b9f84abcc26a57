// state_program.h -- the value-only interpreter of a program on the state of ONE micro element, shared by criterion.hip (one component,
// kept) and secant.hip (n_comp components, each stored where it is formed).  It is the value pass of coef_program.hip's on one element
// instead of a quadrature loop: the dispatch is a scalar branch on readfirstlane of the opcode, every operation one separately rounded
// IEEE operation in program order (hommx_amd.expr.Criterion.host_values / SecantLaw.host_values are its NumPy twins).  The top of the
// stack is a register; the levels below it are rows of dynamic LDS, stack[depth - 1][kWalkThreads], lane-contiguous (no bank conflict; a
// thread touches its own column only: no barrier).  The inputs: x and the 2 t state values are selected by switches on the uniform
// operand over static registers (no register array is indexed dynamically, hence no scratch); a field f[k], y[i] (the element centroid)
// and c[k] are vector loads where they are read.  What STORE does is the caller's: store(k, value), k uniform.
#pragma once
#include <hip/hip_runtime.h>

#include "coef_program.h"
#include "elem_walk.h"

namespace hommx {

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

// The program on one element.  x: the midpoint; row: the cell's row (the fields behind the midpoint); e, s: strain and flux; ce: the
// element's coefficient entry, what c[k] reads; yk: its centroid (read by Y only); stk: this thread's column of the stack rows;
// store(k, v): component k of the element has the value v
template <int T, typename Store>
__device__ __forceinline__ void run_state_program(const ProgramArgs& prog, int n_fields, const double (&x)[3], const double* __restrict__ row,
                                                  const double (&e)[T], const double (&s)[T], const double* __restrict__ ce,
                                                  const double* __restrict__ yk, double* __restrict__ stk, Store&& store) {
#pragma clang fp contract(off)
  const int n_ops = prog.n_ops, base = program_row_doubles(n_fields);
  double t = 0.0;
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
    const uint32_t word = prog.code[pc >> 1] >> ((pc & 1) * 16);  // little endian: opcode in the low byte, operand above it
    const int op = uniform(word & 0xff), k = uniform((word >> 8) & 0xff);
    switch (op) {
      case OP_CONST:
        push();
        t = prog.consts[k];
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
      default:  // OP_STORE k: the validation admits no other opcode
        store(k, t);
        --sp;
        if (sp > 0) t = stk[(sp - 1) * kWalkThreads];
        break;
    }
  }
}

}  // namespace hommx
