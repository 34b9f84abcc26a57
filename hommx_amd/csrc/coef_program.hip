// coef_program.hip -- expression coefficients sampled on the device: a bytecode interpreter expands the program of a
// HOMMX_COEF_PROGRAM source (include/hommx_hip.h; coef_program.h) into the plan's element stream and, in forward mode, into its
// first and second derivatives with respect to the differentiable slots.
//
// ONE interpreter body, expand_body<P, H>: a stack entry is (v, d_0 .. d_{P-1}) and, with H, the second-order slots h_ab of the pairs
// a <= b of those P slots behind them -- (v, d, h) for P = 1, (v, d_0, d_1, h_00, h_01, h_11) for P = 2.  Two kernel templates
// instantiate it: k_expand_program<P> without second order (the value pass is its instantiation without tangents, P = 0) and
// k_expand_program2<P>, P = 1, 2, with it.  Every opcode has one case that states its value rule, its tangent rule and its second-order
// rule; every loop over j (over s) is unrolled over the template parameters and is not there for P = 0 (without H), so one set of
// statements computes `t` and `d` whatever the instantiation is: the value stream of the tangent pass is the value pass's, and the value
// and tangent streams of the second-order pass are the tangent pass's, bit for bit by construction.
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
// program (hommx_amd.expr.Expression.host_stream / host_tangents / host_second_tangents) reproduces the streams bit for bit wherever
// the program contains exactly rounded operations only.
//
// The second-order kernel runs one wave of 64 per block and keeps its stack in DYNAMIC LDS, stack[row][1 + P + S][64] with only the
// rows the program needs (its validated depth, which the launcher is given): 1.5 KiB (P = 1) or 3 KiB (P = 2) per row, 48 KiB at the
// admissible depth of 16.  Behind the rows stand the sums of the second-order slots, acch[n_comp][S][64] (0.5 .. 9 KiB, the same
// conflict-free layout; a STORE adds to S of them): in registers the 6 S doubles took the two-slot kernel to 256 VGPRs + 14 AGPRs, one
// wave per SIMD; in LDS it has 206 and two.  At the 3 .. 6 rows of a typical program registers, not LDS, bound the resident blocks.
//
// The per-cell row is the midpoint and then the n_fields fields of the cell (coef_program.h, program_row_doubles).  The midpoint lives in
// registers; a field does not -- `X k`, k >= 3, loads row[k] where it is read.  The row is 32 .. 56 bytes and stays in cache, the lanes
// of a wave may belong to different cells (a vector load, not a scalar one), and the instantiation of four slots has no registers to
// spare for four more live doubles.  A program without fields never takes that branch.
//
// Forward mode: the differentiable slots are the parameters (the first n_params constants), then the fields (n_tan = n_params + n_fields
// <= P): `CONST k`, k < n_params, seeds slot k, and `X k`, k >= 3, seeds slot n_params + k - 3.  The rules are those of
// include/hommx_hip.h (hommx_expand_tangents, hommx_expand_second_tangents), which hommx_amd.expr._run restates with NumPy.  Where every
// operand's d_j is 0.0 the result's d_j is +0.0 and the formula does not count (rule1 / rule2 below): a sqrt(0) or a division by zero
// in a part of the expression that does not read slot j cannot make its tangent NaN -- and the cosine of SIN (the sine of COS) is not
// evaluated at all by a wave none of whose lanes carries a tangent through the call, nor by the value pass.  The second order has the
// twin of that rule (ruleh1 / ruleh2): h_ab is +0.0 where every operand's h_ab is 0.0 and every operand's d_a, or every operand's
// d_b, is 0.0.
//
// Second order with more than two slots: k_expand_program2<2> runs once per unordered pair {a, b}, a < b, of the program's slots (3 or
// 6 launches), with a wave-uniform slot map -- which two of the program's slots ride in d_0 and d_1 -- and a mask of what to store:
// every launch writes the streams no earlier one has written.
#include "coef_program.h"

#include "kernels.h"

namespace hommx {

namespace {

constexpr int program_block(int P) { return P == 0 ? 256 : P == 4 ? 64 : 128; }
constexpr int kBlock2 = 64;  // the second-order kernel: one wave

// the second-order slots of P first-order ones: their number, and the first-order slots (a, b), a <= b, of slot s -- (0,0), (0,1), (1,1)
constexpr int pair_count(int P) { return P * (P + 1) / 2; }
constexpr int pair_a(int s) { return s == 2 ? 1 : 0; }
constexpr int pair_b(int s) { return s >= 1 ? 1 : 0; }
// the stream of the pair (a, b), a <= b, of n slots in the row-major order of the ABI
__host__ __device__ constexpr int pair_index(int a, int b, int n) { return a * n - a * (a - 1) / 2 + (b - a); }
// what a launch of the second-order kernel stores: bit 0 coef, bit 1 + j the tangent d_j, bit 3 + s the pair s
constexpr int kStoreCoef = 1, kStoreDir = 2, kStorePair = 8;

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ double pick3(int k, double a0, double a1, double a2) { return k == 0 ? a0 : k == 1 ? a1 : a2; }

// The interpreter.  stack(row, c): entry c of row `row` of this thread's column.  Without H the slots are the program's own (slot j
// rides in d_j) and slot0 / slot1 / store are not read; with H, d_0 / d_1 carry the program's slots slot0 / slot1 and `store` says
// which streams this launch writes
template <int P, bool H, int BLK, typename Stack, typename Sums>
__device__ __forceinline__ void expand_body(const ProgramArgs& prog, int n_params, int n_fields, const double* __restrict__ points,
                                            const double* __restrict__ weights, int n_q, int dim, const double* __restrict__ mid,
                                            double* __restrict__ coef, double* __restrict__ dirs, double* __restrict__ curv, long long n_el,
                                            long long total, Stack stack, Sums acch, int slot0, int slot1, int store) {
#pragma clang fp contract(off)
  constexpr int PN = P ? P : 1;  // PN: no array of length zero; what P = 0 declares with it is never touched
  constexpr int S = H ? pair_count(P) : 0, SN = S ? S : 1;
  const int tid = threadIdx.x;
  const long long idx = (long long)blockIdx.x * BLK + tid;
  if (idx >= total) return;  // the tail of the grid; nothing below synchronises
  const long long cell = idx / n_el, el = idx - cell * n_el;
  const double* row = mid + cell * program_row_doubles(n_fields);  // the midpoint, then the fields of the cell
  const double x0 = row[0], x1 = row[1], x2 = row[2];
  const int n_tan = n_params + n_fields;  // the differentiable slots: the parameters, then the fields
  const int slot[2] = {H ? slot0 : 0, H ? slot1 : 1};  // read with H only
  const double* yp = points + el * n_q * dim;
  // the sums of the values and the tangents in registers; those of the second-order slots, acch(c, s), in LDS behind the stack (c <
  // n_comp only): 6 S more doubles in registers would cost the two-slot kernel its second wave per SIMD
  double acc[PROGRAM_MAX_COMP], accd[PROGRAM_MAX_COMP][PN];
#pragma unroll
  for (int c = 0; c < PROGRAM_MAX_COMP; ++c) {
    acc[c] = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) accd[c][j] = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (c < prog.n_comp) acch(c, s) = 0.0;
  }
  const int n_ops = prog.n_ops;
  for (int q = 0; q < n_q; ++q) {
    const double y0 = yp[q * dim], y1 = yp[q * dim + 1], y2 = dim > 2 ? yp[q * dim + 2] : 0.0;
    const double w = weights[q];
    // depth sp: the top is (t, d, h), the entries below it stack[1 .. sp-1][.][tid] (a push at depth 0 parks the dead top in row 0).
    // (da, ha): the tangents of the popped entry; dt: those of the top before the instruction's tangent rule replaced them
    double t = 0.0, d[PN], da[PN], dt[PN], h[SN], ha[SN];
#pragma unroll
    for (int j = 0; j < P; ++j) d[j] = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) h[s] = 0.0;
    int sp = 0;
    auto push = [&] {
      stack(sp, 0) = t;
#pragma unroll
      for (int j = 0; j < P; ++j) stack(sp, 1 + j) = d[j];
#pragma unroll
      for (int s = 0; s < S; ++s) stack(sp, 1 + P + s) = h[s];
      ++sp;
    };
    auto pop = [&]() -> double {  // the entry below the top: its value, its tangents into da (ha)
      --sp;
#pragma unroll
      for (int j = 0; j < P; ++j) da[j] = stack(sp, 1 + j);
#pragma unroll
      for (int s = 0; s < S; ++s) ha[s] = stack(sp, 1 + P + s);
      return stack(sp, 0);
    };
    auto pop_value = [&]() -> double { return stack(--sp, 0); };  // an operand whose tangent does not count
    auto flat = [&] {  // piecewise constant results
#pragma unroll
      for (int j = 0; j < P; ++j) d[j] = 0.0;
#pragma unroll
      for (int s = 0; s < S; ++s) h[s] = 0.0;
    };
    // d_j of a result of one operand (the top) / of two (the popped entry and the top): +0.0 where every operand's d_j is 0.0 and
    // f(j) is then not evaluated, else f(j) -- `rule` of hommx_amd/expr.py
    auto rule1 = [&](auto f) {
#pragma unroll
      for (int j = 0; j < P; ++j) {
        double r = 0.0;
        dt[j] = d[j];
        if (d[j] != 0.0) r = f(j);
        d[j] = r;
      }
    };
    auto rule2 = [&](auto f) {
#pragma unroll
      for (int j = 0; j < P; ++j) {
        double r = 0.0;
        dt[j] = d[j];
        if (da[j] != 0.0 || d[j] != 0.0) r = f(j);
        d[j] = r;
      }
    };
    // h_ab of such a result, after its tangent rule (the operands' tangents are dt and da, d is the result's): +0.0 where every
    // operand's h_ab is 0.0 and every operand's d_a or every operand's d_b is 0.0, and f(s, a, b) is then not evaluated, else
    // f(s, a, b), which reads the top's own h[s] before it is replaced -- `rule_h` of hommx_amd/expr.py
    auto ruleh1 = [&](auto f) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int a = pair_a(s), b = pair_b(s);
        double r = 0.0;
        if (h[s] != 0.0 || (dt[a] != 0.0 && dt[b] != 0.0)) r = f(s, a, b);
        h[s] = r;
      }
    };
    auto ruleh2 = [&](auto f) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int a = pair_a(s), b = pair_b(s);
        double r = 0.0;
        if (ha[s] != 0.0 || h[s] != 0.0 || ((da[a] != 0.0 || dt[a] != 0.0) && (da[b] != 0.0 || dt[b] != 0.0))) r = f(s, a, b);
        h[s] = r;
      }
    };
    auto any_live = [&] {  // does this lane carry a tangent or a second-order slot in the top?  (false for P = 0)
      bool any = false;
#pragma unroll
      for (int j = 0; j < P; ++j) any = any || d[j] != 0.0;
#pragma unroll
      for (int s = 0; s < S; ++s) any = any || h[s] != 0.0;
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
          for (int j = 0; j < P; ++j) d[j] = (k == (H ? slot[j] : j) && k < n_params) ? 1.0 : 0.0;
#pragma unroll
          for (int s = 0; s < S; ++s) h[s] = 0.0;
          break;
        case OP_X:
          push();
          if (k < 3) {
            t = pick3(k, x0, x1, x2);
            flat();
          } else {  // field k - 3, loaded where it is read (uniform k: a scalar branch, a vector load); it seeds its own slot
            t = row[k];
#pragma unroll
            for (int j = 0; j < P; ++j) d[j] = ((H ? slot[j] : j) == n_params + k - 3) ? 1.0 : 0.0;
#pragma unroll
            for (int s = 0; s < S; ++s) h[s] = 0.0;
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
          ruleh2([&](int s, int, int) { return add_rn(ha[s], h[s]); });
          t = add_rn(a, t);
          break;
        }
        case OP_SUB: {
          const double a = pop();
          rule2([&](int j) { return add_rn(da[j], -d[j]); });
          ruleh2([&](int s, int, int) { return add_rn(ha[s], -h[s]); });
          t = add_rn(a, -t);
          break;
        }
        case OP_MUL: {
          const double a = pop();
          rule2([&](int j) { return add_rn(mul_rn(a, d[j]), mul_rn(da[j], t)); });
          ruleh2([&](int s, int i, int j) {
            return add_rn(add_rn(add_rn(mul_rn(a, h[s]), mul_rn(ha[s], t)), mul_rn(da[i], dt[j])), mul_rn(da[j], dt[i]));
          });
          t = mul_rn(a, t);
          break;
        }
        case OP_DIV: {
          const double a = pop(), v = div_rn(a, t);
          rule2([&](int j) { return div_rn(add_rn(da[j], -mul_rn(v, d[j])), t); });
          ruleh2([&](int s, int i, int j) {
            return div_rn(add_rn(add_rn(add_rn(ha[s], -mul_rn(d[i], dt[j])), -mul_rn(d[j], dt[i])), -mul_rn(v, h[s])), t);
          });
          t = v;
          break;
        }
        case OP_NEG:
          rule1([&](int j) { return -d[j]; });
          ruleh1([&](int s, int, int) { return -h[s]; });
          t = -t;
          break;
        case OP_ABS:
          rule1([&](int j) { return t < 0.0 ? -d[j] : d[j]; });
          ruleh1([&](int s, int, int) { return t < 0.0 ? -h[s] : h[s]; });
          t = __builtin_fabs(t);
          break;
        case OP_MIN: {
          const double a = pop();
          const bool top = t < a;
          rule2([&](int j) { return top ? d[j] : da[j]; });
          ruleh2([&](int s, int, int) { return top ? h[s] : ha[s]; });
          t = top ? t : a;
          break;
        }
        case OP_MAX: {
          const double a = pop();
          const bool top = t > a;
          rule2([&](int j) { return top ? d[j] : da[j]; });
          ruleh2([&](int s, int, int) { return top ? h[s] : ha[s]; });
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
          ruleh2([&](int s, int, int) { return first ? ha[s] : h[s]; });
          t = first ? a : t;
          break;
        }
        case OP_SQRT:
          t = ::sqrt(t);
          rule1([&](int j) { return div_rn(d[j], mul_rn(2.0, t)); });
          ruleh1([&](int s, int i, int j) { return div_rn(add_rn(h[s], -mul_rn(mul_rn(2.0, d[i]), d[j])), mul_rn(2.0, t)); });
          break;
        case OP_SIN: {
          double c = 0.0;
          if (any_live()) c = ::cos(t);
          rule1([&](int j) { return mul_rn(c, d[j]); });
          t = ::sin(t);
          ruleh1([&](int s, int i, int j) { return add_rn(mul_rn(c, h[s]), -mul_rn(mul_rn(t, dt[i]), dt[j])); });
          break;
        }
        case OP_COS: {
          double s = 0.0;
          if (any_live()) s = ::sin(t);
          rule1([&](int j) { return -mul_rn(s, d[j]); });
          t = ::cos(t);
          ruleh1([&](int r, int i, int j) { return add_rn(-mul_rn(s, h[r]), -mul_rn(mul_rn(t, dt[i]), dt[j])); });
          break;
        }
        case OP_TAN: {
          t = ::tan(t);
          const double g = add_rn(1.0, mul_rn(t, t));
          rule1([&](int j) { return mul_rn(d[j], g); });
          ruleh1([&](int s, int i, int j) { return add_rn(mul_rn(g, h[s]), mul_rn(mul_rn(mul_rn(2.0, t), d[j]), dt[i])); });
          break;
        }
        case OP_EXP:
          t = ::exp(t);
          rule1([&](int j) { return mul_rn(t, d[j]); });
          ruleh1([&](int s, int i, int j) { return add_rn(mul_rn(t, h[s]), mul_rn(d[j], dt[i])); });
          break;
        case OP_LOG:
          rule1([&](int j) { return div_rn(d[j], t); });
          ruleh1([&](int s, int i, int j) { return div_rn(add_rn(h[s], -mul_rn(dt[i], d[j])), t); });
          t = ::log(t);
          break;
        case OP_TANH: {
          t = ::tanh(t);
          const double g = add_rn(1.0, -mul_rn(t, t));
          rule1([&](int j) { return mul_rn(d[j], g); });
          ruleh1([&](int s, int i, int j) { return add_rn(mul_rn(g, h[s]), -mul_rn(mul_rn(mul_rn(2.0, t), d[j]), dt[i])); });
          break;
        }
        default: {  // OP_STORE: the validation admits no other opcode
          const double v = mul_rn(w, t);
          auto add_to = [&](int c) {  // inlined with a constant c: no register array is indexed dynamically
            acc[c] = add_rn(acc[c], v);
#pragma unroll
            for (int j = 0; j < P; ++j) accd[c][j] = add_rn(accd[c][j], mul_rn(w, d[j]));
#pragma unroll
            for (int s = 0; s < S; ++s) acch(c, s) = add_rn(acch(c, s), mul_rn(w, h[s]));
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
#pragma unroll
          for (int s = 0; s < S; ++s) h[s] = ha[s];
          break;
        }
      }
    }
  }
  const int n_comp = prog.n_comp;
#pragma unroll
  for (int c = 0; c < PROGRAM_MAX_COMP; ++c)
    if (c < n_comp) {
      if constexpr (!H) {
        if (coef) coef[idx * n_comp + c] = acc[c];
#pragma unroll
        for (int j = 0; j < P; ++j)
          if (j < n_tan) dirs[((cell * n_tan + j) * n_el + el) * n_comp + c] = accd[c][j];
      } else {  // what this launch is to store: slot[j] < n_tan and the pair of two such slots is below n_pairs
        const int n_pairs = n_tan * (n_tan + 1) / 2;
        if (coef && (store & kStoreCoef)) coef[idx * n_comp + c] = acc[c];
#pragma unroll
        for (int j = 0; j < P; ++j)
          if (dirs && (store & (kStoreDir << j))) dirs[((cell * n_tan + slot[j]) * n_el + el) * n_comp + c] = accd[c][j];
#pragma unroll
        for (int s = 0; s < S; ++s)
          if (store & (kStorePair << s))
            curv[((cell * n_pairs + pair_index(slot[pair_a(s)], slot[pair_b(s)], n_tan)) * n_el + el) * n_comp + c] = acch(c, s);
      }
    }
}

template <int P>
__global__ __launch_bounds__(program_block(P)) void k_expand_program(const ProgramArgs prog, int n_params, int n_fields,
                                                                     const double* __restrict__ points,
                                                                     const double* __restrict__ weights, int n_q, int dim,
                                                                     const double* __restrict__ mid, double* __restrict__ coef,
                                                                     double* __restrict__ dirs, long long n_el, long long total) {
  constexpr int BLK = program_block(P);
  __shared__ double stack[PROGRAM_MAX_STACK][1 + P][BLK];
  const int tid = threadIdx.x;
  expand_body<P, false, BLK>(prog, n_params, n_fields, points, weights, n_q, dim, mid, coef, dirs, nullptr, n_el, total,
                             [&](int r, int c) -> double& { return stack[r][c][tid]; },
                             [&](int, int) -> double& { return stack[0][0][tid]; } /* no second order: never called */, 0, 1, 0);
}

// the second-order pass: d_0 / d_1 carry the program's slots slot0 / slot1 (P = 1: slot0 = 0), `store` the streams of this launch;
// dynamic LDS: the stack of `depth` rows, [row][1 + P + S][64], then the sums of the second-order slots, [n_comp][S][64]
template <int P>
__global__ __launch_bounds__(kBlock2) void k_expand_program2(const ProgramArgs prog, int n_params, int n_fields,
                                                             const double* __restrict__ points, const double* __restrict__ weights,
                                                             int n_q, int dim, const double* __restrict__ mid, double* __restrict__ coef,
                                                             double* __restrict__ dirs, double* __restrict__ curv, long long n_el,
                                                             long long total, int depth, int slot0, int slot1, int store) {
  constexpr int S = pair_count(P), W = 1 + P + S;
  extern __shared__ double stack2[];
  const int tid = threadIdx.x;
  double* sums = stack2 + depth * W * kBlock2;
  expand_body<P, true, kBlock2>(prog, n_params, n_fields, points, weights, n_q, dim, mid, coef, dirs, curv, n_el, total,
                                [&](int r, int c) -> double& { return stack2[(r * W + c) * kBlock2 + tid]; },
                                [&](int c, int s) -> double& { return sums[(c * S + s) * kBlock2 + tid]; }, slot0, slot1, store);
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

hipError_t launch_expand_program2(const ProgramArgs& prog, int n_params, int n_fields, int depth, const double* d_points,
                                  const double* d_weights, int n_q, int dim, const double* d_rows, double* d_coef, double* d_dirs,
                                  double* d_curv, long long n_el, long long ncells, hipStream_t stream) {
  const long long total = ncells * n_el;
  const int n_tan = n_params + n_fields;
  if (total <= 0) return hipSuccess;
  if (n_tan < 1 || n_tan > PROGRAM_MAX_PARAMS || depth < 1 || depth > PROGRAM_MAX_STACK || !d_curv) return hipErrorInvalidValue;
  auto launch = [&](auto kernel, int P, int slot0, int slot1, int store) {
    const size_t lds = sizeof(double) * (depth * (1 + P + pair_count(P)) + prog.n_comp * pair_count(P)) * kBlock2;  // at most 57 KiB
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + kBlock2 - 1) / kBlock2)), dim3(kBlock2), lds, stream, prog, n_params, n_fields,
                       d_points, d_weights, n_q, dim, d_rows, d_coef, d_dirs, d_curv, n_el, total, depth, slot0, slot1, store);
  };
  if (n_tan == 1) {
    launch(k_expand_program2<1>, 1, 0, 0, kStoreCoef | kStoreDir | kStorePair);
    return hipGetLastError();
  }
  // one launch per pair of slots a < b; a launch stores the value, the tangents and the pairs no earlier launch has stored
  bool have_dir[PROGRAM_MAX_PARAMS] = {}, have_pair[PROGRAM_MAX_PARAMS][PROGRAM_MAX_PARAMS] = {};
  bool have_coef = false;
  for (int a = 0; a < n_tan; ++a)
    for (int b = a + 1; b < n_tan; ++b) {
      const int sl[2] = {a, b};
      int store = have_coef ? 0 : kStoreCoef;
      have_coef = true;
      for (int j = 0; j < 2; ++j)
        if (!have_dir[sl[j]]) {
          store |= kStoreDir << j;
          have_dir[sl[j]] = true;
        }
      for (int s = 0; s < 3; ++s)
        if (bool& have = have_pair[sl[pair_a(s)]][sl[pair_b(s)]]; !have) {
          store |= kStorePair << s;
          have = true;
        }
      launch(k_expand_program2<2>, 2, a, b, store);
    }
  return hipGetLastError();
}

}  // namespace hommx
