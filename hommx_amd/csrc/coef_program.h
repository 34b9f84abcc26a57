// coef_program.h -- the bytecode of an expression coefficient (include/hommx_hip.h, HOMMX_COEF_PROGRAM): what api.hip validates on the
// host and coef_program.hip interprets on the device.  hommx_amd/expr.py writes the same numbers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hommx {

// A postfix program over a stack of doubles.  Every instruction is (opcode, operand); the operand is the index of CONST / X / Y / STORE
// and unused otherwise.  A comparison leaves 1.0 or 0.0; AND / OR / NOT / SELECT read "non-zero" as true; SELECT takes (c, a, b), b on
// top, and leaves c ? a : b, both evaluated; MIN / MAX leave (b < a ? b : a) / (b > a ? b : a) for (a, b), b on top; STORE c pops the
// value of component c at this quadrature point
enum CoefOp : uint8_t {
  OP_CONST = 0, OP_X, OP_Y, OP_ADD, OP_SUB, OP_MUL, OP_DIV, OP_NEG, OP_ABS, OP_MIN, OP_MAX, OP_LT, OP_LE, OP_GT, OP_GE, OP_AND, OP_OR,
  OP_NOT, OP_SELECT, OP_SQRT, OP_SIN, OP_COS, OP_TAN, OP_EXP, OP_LOG, OP_TANH, OP_DUP, OP_STORE, OP_COUNT
};
constexpr int PROGRAM_MAX_OPS = 128, PROGRAM_MAX_CONSTS = 32, PROGRAM_MAX_STACK = 16, PROGRAM_MAX_COMP = 6;

// values an instruction takes from the stack / leaves on it
constexpr int op_pops(int op) {
  return op <= OP_Y ? 0 : op == OP_SELECT ? 3 : (op == OP_NEG || op == OP_ABS || op == OP_NOT || (op >= OP_SQRT && op <= OP_STORE)) ? 1 : 2;
}
constexpr int op_pushes(int op) { return op == OP_STORE ? 0 : op == OP_DUP ? 2 : 1; }

// the program as the kernel takes it, by value in its arguments (wave-uniform: scalar loads).  code: the bytes of ops[n_ops][2], two
// instructions per 32-bit word, so that the fetch is an aligned s_load_dword (a byte pair compiles to a vector global_load_ushort)
struct ProgramArgs {
  uint32_t code[PROGRAM_MAX_OPS / 2];
  double consts[PROGRAM_MAX_CONSTS];
  int n_ops = 0, n_comp = 0;
};

// The per-cell row of a program source (hommx_coef_source.params): the midpoint of the macro cell, then its n_fields fields
// (include/hommx_hip.h, HOMMX_PROGRAM_MAX_FIELDS); `X k` reads entry k of the row.  THE place that knows the width of the row: the
// host (api.hip: staging, chunk offsets) and the kernel stride by it
constexpr int PROGRAM_MAX_FIELDS = 4;
__host__ __device__ constexpr int program_row_doubles(int n_fields) { return 3 + n_fields; }

// The parameters of a program are its first n_params constants (include/hommx_hip.h, HOMMX_PROGRAM_MAX_PARAMS); the differentiable
// slots of the forward mode are the parameters, then the fields, at most PROGRAM_MAX_PARAMS together
constexpr int PROGRAM_MAX_PARAMS = 4;

// coef_program.hip: coef[cell][el][comp] = sum_q w[q] * program(x = rows[cell], y = points[el][q]) as separately rounded operations,
// q ascending from 0 (d_coef; null: not written), and with d_dirs, in the same pass, its derivatives with respect to the parameters and
// the fields, dirs[cell][j][el][comp], j < n_params + n_fields (1 .. PROGRAM_MAX_PARAMS), by the rules of include/hommx_hip.h
// (hommx_expand_tangents).  d_dirs null: the value pass, whatever slots the program has; both passes are instantiations of one kernel
// and give the same coef bit for bit.  points [n_el][n_q][dim], weights [n_q], rows [ncells][program_row_doubles(n_fields)], all on the
// device; `prog` has passed the host validation
hipError_t launch_expand_program(const ProgramArgs& prog, int n_params, int n_fields, const double* d_points, const double* d_weights,
                                 int n_q, int dim, const double* d_rows, double* d_coef, double* d_dirs, long long n_el, long long ncells,
                                 hipStream_t stream);

// The second-order forward mode, in the same pass: curv[cell][pair][el][comp] = d2 coef / d slot_a d slot_b for the pairs (a, b),
// a <= b, of the n_tan = n_params + n_fields slots in row-major order -- (0,0), (0,1), .., (0,n-1), (1,1), .. --, n_pairs =
// n_tan (n_tan + 1) / 2, by the rules of include/hommx_hip.h (hommx_expand_second_tangents).  d_coef and d_dirs as above, both optional
// here, and where given the bits launch_expand_program writes.  depth: the maximal stack depth of the program (1 .. PROGRAM_MAX_STACK),
// which with prog.n_comp sizes the kernel's dynamic LDS.  One launch for n_tan <= 2, one per pair of slots a < b for n_tan = 3, 4
hipError_t launch_expand_program2(const ProgramArgs& prog, int n_params, int n_fields, int depth, const double* d_points,
                                  const double* d_weights, int n_q, int dim, const double* d_rows, double* d_coef, double* d_dirs,
                                  double* d_curv, long long n_el, long long ncells, hipStream_t stream);

}  // namespace hommx
