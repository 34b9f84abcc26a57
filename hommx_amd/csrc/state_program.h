// state_program.h -- the interpreter of a program on the state of ONE micro element, shared by criterion.hip (one component, kept),
// secant.hip (n_comp components, each stored where it is formed) and, in forward mode over the strain, secant_tangent.hip.  It is the
// value pass of coef_program.hip's on one element instead of a quadrature loop: the dispatch is a scalar branch on readfirstlane of the
// opcode, every operation one separately rounded IEEE operation in program order (hommx_amd.expr.Criterion.host_values /
// SecantLaw.host_values are its NumPy twins).  The top of the stack is a register; the levels below it are rows of dynamic LDS,
// stack[depth - 1][kWalkThreads], lane-contiguous (no bank conflict; a thread touches its own column only: no barrier).  The inputs: x and
// the 2 t state values are selected by switches on the uniform operand over static registers (no register array is indexed dynamically,
// hence no scratch); a field f[k], y[i] (the element centroid) and c[k] are vector loads where they are read.  What STORE does is the
// caller's: store(k, value), k uniform.
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
//
// P > 0: the forward mode over P slots, in the manner of coef_program.hip's expand_body<P, H>.  A stack entry is (v, d_0 .. d_{P-1}),
// the rows are stack[depth - 1][1 + P][kWalkThreads], and the seeds are the state reads: `X base + n` of the strain entries
// n = seed0 .. seed0 + P - 1 of the current sweep seeds d_{n - seed0} = 1, every other read seeds 0.  Each case states its value rule
// and its tangent rule, those of the table in DESIGN.md section 3 (hommx_amd/expr.py, _TANGENT), the dead rule included: d_j of a
// result is +0.0 where every operand's d_j is 0.0, and the formula is then not evaluated.  The value statements do not read a tangent,
// so v is the value pass's bit for bit in every sweep.  store(k, v, d) then.  P = 0 declares no tangent and is the value pass
//
// HIST: the law has history variables.  The row is longer by them: an `X` index at or above
// base + 2 T + n_comp is h[k], a vector load from he, the element's history row, where it is read, as c[k] is; it seeds nothing.
// n_comp: the entries of ce (uniform).  What a STORE k, k >= n_comp, does is the caller's.  Without HIST neither is read, and the
// instantiation is the one it was
//
// BASE (with HIST): a criterion of the nonlinear state (criterion_state.hip).  The row holds a second
// coefficient segment behind the n_history (uniform, 0: none, and he may be null) history entries: an `X` index at or above
// base + 2 T + n_comp + n_history is b[k], a vector load from be, the element's entry of the base stream, where it is read.  Without
// BASE neither is read, and the instantiation is the one it was
template <int T, int P = 0, bool HIST = false, bool BASE = false, typename Store>
__device__ __forceinline__ void run_state_program(const ProgramArgs& prog, int n_fields, const double (&x)[3], const double* __restrict__ row,
                                                  const double (&e)[T], const double (&s)[T], const double* __restrict__ ce,
                                                  const double* __restrict__ yk, double* __restrict__ stk, Store&& store, int seed0 = 0,
                                                  const double* __restrict__ he = nullptr, int n_comp = 0,
                                                  const double* __restrict__ be = nullptr, int n_history = 0) {
#pragma clang fp contract(off)
  constexpr int PN = P ? P : 1, W = 1 + P;  // PN: no array of length zero; W: the doubles of a stack entry
  const int n_ops = prog.n_ops, base = program_row_doubles(n_fields);
  double t = 0.0, d[PN], da[PN];  // the top; da: the tangents of the popped entry
#pragma unroll
  for (int j = 0; j < P; ++j) d[j] = 0.0;
  int sp = 0;  // depth: the top is (t, d), the levels below it stk[0 .. sp-2]
  auto push = [&] {
    if (sp > 0) {
      stk[(sp - 1) * W * kWalkThreads] = t;
#pragma unroll
      for (int j = 0; j < P; ++j) stk[((sp - 1) * W + 1 + j) * kWalkThreads] = d[j];
    }
    ++sp;
  };
  auto pop = [&]() -> double {  // the entry below the top: its value, its tangents into da
    --sp;
#pragma unroll
    for (int j = 0; j < P; ++j) da[j] = stk[((sp - 1) * W + 1 + j) * kWalkThreads];
    return stk[(sp - 1) * W * kWalkThreads];
  };
  auto pop_value = [&]() -> double {  // an operand whose tangent does not count
    --sp;
    return stk[(sp - 1) * W * kWalkThreads];
  };
  auto flat = [&] {  // a read that seeds nothing, a piecewise constant result
#pragma unroll
    for (int j = 0; j < P; ++j) d[j] = 0.0;
  };
  auto rule1 = [&](auto f) {  // d_j of a result of one operand, the top
#pragma unroll
    for (int j = 0; j < P; ++j) {
      double r = 0.0;
      if (d[j] != 0.0) r = f(j);
      d[j] = r;
    }
  };
  auto rule2 = [&](auto f) {  // ... of two, the popped entry and the top
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
        flat();
        break;
      case OP_X:
        push();
        flat();
        if (k < 3) {
          t = pick<3>(k, x);
        } else if (k < base) {
          t = row[k];
        } else if (k < base + T) {
          t = pick<T>(k - base, e);
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = k - base == seed0 + j ? 1.0 : 0.0;
        } else if (k < base + 2 * T) {
          t = pick<T>(k - base - T, s);
        } else if (!HIST || k < base + 2 * T + n_comp) {
          t = ce[k - base - 2 * T];
        } else if (!BASE || k < base + 2 * T + n_comp + n_history) {
          if constexpr (HIST) t = he[k - base - 2 * T - n_comp];
        } else {
          if constexpr (BASE) t = be[k - base - 2 * T - n_comp - n_history];
        }
        break;
      case OP_Y:
        push();
        t = yk[k];
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
        double c = 0.0;
        if (any_live()) c = ::sin(t);
        rule1([&](int j) { return -mul_rn(c, d[j]); });
        t = ::cos(t);
        break;
      }
      case OP_TAN: {
        t = ::tan(t);
        if constexpr (P > 0) {
          const double g = add_rn(1.0, mul_rn(t, t));
          rule1([&](int j) { return mul_rn(d[j], g); });
        }
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
        if constexpr (P > 0) {
          const double g = add_rn(1.0, -mul_rn(t, t));
          rule1([&](int j) { return mul_rn(d[j], g); });
        }
        break;
      }
      default:  // OP_STORE k: the validation admits no other opcode
        if constexpr (P > 0)
          store(k, t, d);
        else
          store(k, t);
        --sp;
        if (sp > 0) {
          t = stk[(sp - 1) * W * kWalkThreads];
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] = stk[((sp - 1) * W + 1 + j) * kWalkThreads];
        }
        break;
    }
  }
}

}  // namespace hommx
