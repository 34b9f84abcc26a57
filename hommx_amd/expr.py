"""Expression coefficients: ``A(x, y)`` written as text, compiled to a small postfix program that the library interprets on the device
(include/hommx_hip.h, HOMMX_COEF_PROGRAM; csrc/coef_program.hip) and this module interprets with NumPy -- the same operations in the same
order on both sides.

The text is parsed with ``ast`` and never evaluated by Python.  Grammar: the names ``x[0..2]`` (macro cell midpoint), ``y[0..d-1]`` (fast
variable), ``p[0..3]`` (a parameter, its value given with ``Expression(..., p=[...])``), ``f[0..3]`` (a field: one value per macro
cell, admitted with ``Expression(..., fields=...)``) and ``pi``, numeric literals, ``+ - * /``, unary
``-``, ``**`` with a literal integer exponent 0 .. 8, the comparisons ``< <= > >=`` with ``and`` / ``or`` / ``not`` on them, and the
calls ``abs min max where(c, a, b) sqrt sin cos tan exp log tanh``.

Because the library can read the expression, its quadrature degree is estimated from the tree by the rules of UFL's degree estimation
(recalled here, UFL is not a dependency): see ``Expression.degree``.

Parameters are the first constants of the program (``p[k]`` is ``CONST k``), so every path that takes a program takes one with
parameters.  The library also differentiates the program with respect to them in forward mode -- the value pass is the instantiation
of its one interpreter kernel without differentiable slots (csrc/coef_program.hip, ``k_expand_program<P>``), and ``_run`` here is
built the same way; ``Expression.host_tangents`` is the NumPy twin of the forward-mode pass: the rules of ``_TANGENT``, the same
operations in the same order.  The second-order pass (``k_expand_program2<P>``, the same interpreter body) has its twin in
``Expression.host_second_tangents`` and the rules of ``_TANGENT2``.

Fields are read like the midpoint: ``f[k]`` is ``X 3 + k``, entry ``3 + k`` of the cell's row, so everywhere in this module they ride
as extra rows of ``x`` (``x[3 + n_fields, ...]``), and every path that takes a program takes one with fields.  They are differentiated
like parameters; the differentiable slots are the parameters, then the fields.
"""

from __future__ import annotations

import ast
import copy
import logging
import math

import numpy as np

# opcodes of the program (the OP_* of csrc/coef_program.h, which the kernel and the host validation share)
(OP_CONST, OP_X, OP_Y, OP_ADD, OP_SUB, OP_MUL, OP_DIV, OP_NEG, OP_ABS, OP_MIN, OP_MAX, OP_LT, OP_LE, OP_GT, OP_GE, OP_AND, OP_OR, OP_NOT,
 OP_SELECT, OP_SQRT, OP_SIN, OP_COS, OP_TAN, OP_EXP, OP_LOG, OP_TANH, OP_DUP, OP_STORE) = range(28)
MAX_OPS, MAX_CONSTS, MAX_STACK, MAX_COMP = 128, 32, 16, 6
MAX_POWER = 8
MAX_PARAMS = 4  # HOMMX_PROGRAM_MAX_PARAMS
MAX_FIELDS = 4  # HOMMX_PROGRAM_MAX_FIELDS
MAX_LAW_COMP = 21  # the components of a SecantLaw: the entries of the coefficient of an element, 21 on the 3D Voigt kind
MAX_HISTORY = 4  # HOMMX_SECANT_MAX_HISTORY: the history variables h[k] of a SecantLaw

_BINARY = {ast.Add: OP_ADD, ast.Sub: OP_SUB, ast.Mult: OP_MUL, ast.Div: OP_DIV}
_COMPARE = {ast.Lt: OP_LT, ast.LtE: OP_LE, ast.Gt: OP_GT, ast.GtE: OP_GE}
_MATH = {"sqrt": OP_SQRT, "sin": OP_SIN, "cos": OP_COS, "tan": OP_TAN, "exp": OP_EXP, "log": OP_LOG, "tanh": OP_TANH}
_MATH_NUMPY = {OP_SQRT: np.sqrt, OP_SIN: np.sin, OP_COS: np.cos, OP_TAN: np.tan, OP_EXP: np.exp, OP_LOG: np.log, OP_TANH: np.tanh}
# what an instruction takes from the stack and leaves on it
_POPS = {OP_CONST: 0, OP_X: 0, OP_Y: 0, OP_DUP: 1, OP_NEG: 1, OP_ABS: 1, OP_NOT: 1, OP_SELECT: 3, OP_STORE: 1}
_POPS.update({op: 1 for op in _MATH.values()})
_PUSHES = {OP_DUP: 2, OP_STORE: 0}
_INF = float("inf")


def _bad(node, why: str):
    what = type(node).__name__
    try:
        what += f" '{ast.unparse(node)}'"
    except Exception:  # pragma: no cover - unparse takes every node the parser makes
        pass
    return ValueError(f"expression: {why}: {what}")


class _Node:
    """One node of the checked tree: ``op`` with ``args`` (nodes) or a leaf (``value``: the constant, or the index of x / y / p);
    ``boolean``: a comparison or a combination of comparisons; ``degree``: the estimate of the module docstring; ``varying``: depends on
    x, y, a parameter or a field (a subtree that does not is folded into one constant); ``p_degree``: the degree in the parameters
    and fields (``Expression.p_degree``)."""

    __slots__ = ("op", "args", "value", "boolean", "degree", "varying", "power", "p_degree")

    def __init__(self, op, args=(), value=None, boolean=False, degree=0, varying=False, power=0, p_degree=0):
        self.op, self.args, self.value, self.boolean, self.degree, self.varying, self.power = op, tuple(args), value, boolean, degree, varying, power
        self.p_degree = p_degree

    def key(self):
        """Structural identity (the off-diagonal texts of a matrix must parse to equal trees)."""
        v = np.float64(self.value).tobytes() if self.op == OP_CONST else self.value
        return (self.op, v, self.power, tuple(a.key() for a in self.args))


_POW = -1  # a node of the tree only: the program spells it DUP / MUL
_PARAM = -2  # p[k], a node of the tree only: the program spells it CONST k (the parameters are the first constants)
_FIELD = -3  # f[k], a node of the tree only: the program spells it X 3 + k (the fields stand after the midpoint in the cell's row)
_STATE = -4  # e[k], s[k] or c[k] of a Criterion, a node of the tree only (value: the name and k): ``X`` on the wider row, once t is known
MAX_STATE_INDEX = 20  # the largest index a state name can have on any plan (c[20]: the 21 Voigt entries)


class _Context:
    """What the components of one Expression share while they are checked: the number of parameters (None: no ``p=``), of fields
    (None: no ``fields=``) and the texts of the comparisons that read one.  ``state``: the text is a ``Criterion``'s, which also
    reads the element's strain ``e[k]``, flux ``s[k]`` and coefficient ``c[k]``.  ``n_history``: the history variables ``h[k]`` of a
    ``SecantLaw`` or of a state ``Criterion`` (None: no ``history=``).  ``base``: the text is a ``Criterion``'s, which may also read
    the base coefficient ``b[k]``."""

    def __init__(self, n_params=None, n_fields=None, state=False, n_history=None, base=False):
        self.n_params, self.n_fields, self.compared, self.state, self.n_history = n_params, n_fields, [], state, n_history
        self.base = base


def _number(node, value) -> _Node:
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise _bad(node, "only numeric literals are allowed")
    return _Node(OP_CONST, value=float(value))


def _literal_int(node, lo: int, hi: int) -> bool:
    return isinstance(node, ast.Constant) and isinstance(node.value, int) and not isinstance(node.value, bool) and lo <= node.value <= hi


def _check(node, ctx: _Context) -> _Node:
    """ast node -> checked tree; anything outside the grammar raises ValueError naming the node."""
    if isinstance(node, ast.Constant):
        return _number(node, node.value)
    if isinstance(node, ast.Name):
        if node.id == "pi":
            return _Node(OP_CONST, value=math.pi)
        raise _bad(node, "unknown name (x[i], y[i] and pi are the names)")
    if isinstance(node, ast.Subscript):
        if isinstance(node.value, ast.Name) and node.value.id == "p" and ctx.n_params is not None:
            if not _literal_int(node.slice, 0, ctx.n_params - 1):
                raise _bad(node, f"the index of p is a literal integer below the number of parameters ({ctx.n_params})")
            return _Node(_PARAM, value=int(node.slice.value), varying=True, p_degree=1)
        if isinstance(node.value, ast.Name) and node.value.id == "p":
            raise _bad(node, "p[k] needs the values of the parameters (p=[...])")
        if isinstance(node.value, ast.Name) and node.value.id == "f" and ctx.n_fields is not None:
            if not _literal_int(node.slice, 0, ctx.n_fields - 1):
                raise _bad(node, f"the index of f is a literal integer below the number of fields ({ctx.n_fields})")
            return _Node(_FIELD, value=int(node.slice.value), varying=True, p_degree=1)
        if ctx.state and isinstance(node.value, ast.Name) and node.value.id in ("e", "s", "c"):
            if not _literal_int(node.slice, 0, MAX_STATE_INDEX):
                raise _bad(node, f"the index of {node.value.id} is a literal integer 0 .. {MAX_STATE_INDEX}")
            return _Node(_STATE, value=(node.value.id, int(node.slice.value)), degree=1, varying=True)
        if ctx.state and ctx.base and isinstance(node.value, ast.Name) and node.value.id == "b":
            if not _literal_int(node.slice, 0, MAX_STATE_INDEX):
                raise _bad(node, f"the index of b is a literal integer 0 .. {MAX_STATE_INDEX}")
            return _Node(_STATE, value=("b", int(node.slice.value)), degree=1, varying=True)
        if ctx.state and isinstance(node.value, ast.Name) and node.value.id == "h":
            if ctx.n_history is None:
                raise _bad(node, "h[k] needs the updates of the history variables (history=[...])")
            if not _literal_int(node.slice, 0, ctx.n_history - 1):
                raise _bad(node, f"the index of h is a literal integer below the number of history variables ({ctx.n_history})")
            return _Node(_STATE, value=("h", int(node.slice.value)), degree=1, varying=True)
        if not (isinstance(node.value, ast.Name) and node.value.id in ("x", "y")):
            raise _bad(node, "only x and y are indexed")
        if not _literal_int(node.slice, 0, 2):
            raise _bad(node, "the index of x and y is a literal 0, 1 or 2")
        fast = node.value.id == "y"
        return _Node(OP_Y if fast else OP_X, value=int(node.slice.value), degree=1 if fast else 0, varying=True)
    if isinstance(node, ast.UnaryOp):
        a = _check(node.operand, ctx)
        if isinstance(node.op, ast.USub):
            return _Node(OP_NEG, [_numeric(a, node)], degree=a.degree, varying=a.varying, p_degree=a.p_degree)
        if isinstance(node.op, ast.UAdd):
            return _numeric(a, node)
        if isinstance(node.op, ast.Not):
            return _Node(OP_NOT, [_logical(a, node)], boolean=True, varying=a.varying)
        raise _bad(node, "unknown unary operator")
    if isinstance(node, ast.BinOp):
        if isinstance(node.op, ast.Pow):
            a = _numeric(_check(node.left, ctx), node)
            k = node.right
            if not _literal_int(k, 0, MAX_POWER):
                raise _bad(node, f"the exponent of ** is a literal integer 0 .. {MAX_POWER}")
            return _Node(_POW, [a], power=int(k.value), degree=k.value * a.degree, varying=a.varying and k.value > 0,
                         p_degree=k.value * a.p_degree if k.value else 0)
        if type(node.op) not in _BINARY:
            raise _bad(node, "unknown binary operator")
        a, b = _numeric(_check(node.left, ctx), node), _numeric(_check(node.right, ctx), node)
        op = _BINARY[type(node.op)]
        degree = max(a.degree, b.degree) if op in (OP_ADD, OP_SUB) else a.degree + b.degree
        if op in (OP_ADD, OP_SUB):
            p_degree = max(a.p_degree, b.p_degree)
        elif op == OP_MUL:
            p_degree = a.p_degree + b.p_degree
        else:  # a quotient is a polynomial in the parameters only over a denominator without them
            p_degree = a.p_degree if b.p_degree == 0 else _INF
        return _Node(op, [a, b], degree=degree, varying=a.varying or b.varying, p_degree=p_degree)
    if isinstance(node, ast.Compare):
        if len(node.ops) != 1 or type(node.ops[0]) not in _COMPARE:
            raise _bad(node, "a comparison is one of < <= > >= between two values")
        a, b = _numeric(_check(node.left, ctx), node), _numeric(_check(node.comparators[0], ctx), node)
        if a.p_degree or b.p_degree:
            ctx.compared.append(ast.unparse(node))
        return _Node(_COMPARE[type(node.ops[0])], [a, b], boolean=True, varying=a.varying or b.varying)
    if isinstance(node, ast.BoolOp):
        op = OP_AND if isinstance(node.op, ast.And) else OP_OR
        parts = [_logical(_check(v, ctx), node) for v in node.values]
        out = parts[0]
        for p in parts[1:]:  # left to right, as Python evaluates them
            out = _Node(op, [out, p], boolean=True, varying=out.varying or p.varying)
        return out
    if isinstance(node, ast.Call):
        if not isinstance(node.func, ast.Name) or node.keywords:
            raise _bad(node, "unknown call")
        name, args = node.func.id, [_check(a, ctx) for a in node.args]
        varying = any(a.varying for a in args)
        kinked = _INF if any(a.p_degree for a in args) else 0  # abs, min, max and the math functions are no polynomials
        if name == "abs" and len(args) == 1:
            return _Node(OP_ABS, [_numeric(args[0], node)], degree=args[0].degree, varying=varying, p_degree=kinked)
        if name in ("min", "max") and len(args) == 2:
            a, b = _numeric(args[0], node), _numeric(args[1], node)
            return _Node(OP_MIN if name == "min" else OP_MAX, [a, b], degree=max(a.degree, b.degree), varying=varying, p_degree=kinked)
        if name == "where" and len(args) == 3:
            c, a, b = _logical(args[0], node), _numeric(args[1], node), _numeric(args[2], node)
            return _Node(OP_SELECT, [c, a, b], degree=max(a.degree, b.degree), varying=varying,
                         p_degree=max(a.p_degree, b.p_degree))  # the condition does not count
        if name in _MATH and len(args) == 1:
            a = _numeric(args[0], node)
            return _Node(_MATH[name], [a], degree=0 if a.degree == 0 else a.degree + 2, varying=varying, p_degree=kinked)
        raise _bad(node, "unknown call (abs min max where sqrt sin cos tan exp log tanh are the calls)")
    raise _bad(node, "not part of the expression grammar")


def _numeric(n: _Node, at) -> _Node:
    if n.boolean:
        raise _bad(at, "a comparison is used as a value (use where(c, a, b))")
    return n


def _logical(n: _Node, at) -> _Node:
    if not n.boolean:
        raise _bad(at, "and / or / not and the condition of where take comparisons")
    return n


def _parse(text, ctx: _Context | None = None) -> _Node:
    if isinstance(text, (int, float)) and not isinstance(text, bool):
        text = repr(float(text))
    if not isinstance(text, str):
        raise ValueError(f"expression: a component is a text; got {type(text).__name__}")
    try:
        tree = ast.parse(text.strip(), mode="eval")
    except SyntaxError as e:
        raise ValueError(f"expression: cannot parse {text!r}: {e.msg}") from None
    return _numeric(_check(tree.body, ctx or _Context()), tree.body)


def _emit(n: _Node, ops: list, consts: list, n_params: int = 0):
    """Postfix code of a tree.  A subtree without x, y and p is one constant: the value this module's own interpreter gives it, so
    literals fold exactly where Python's evaluation order brings two of them together (``2*pi*y[0]`` holds the constant 2 pi;
    ``y[0]*2*pi`` none).  Equal constants share a slot, but never one of the first ``n_params``: those are the parameters."""
    if not n.varying and not n.boolean:
        if n.op == OP_CONST:
            value = n.value
        else:
            sub_ops, sub_consts = [], []
            _emit_plain(n, sub_ops, sub_consts, 0)
            sub_ops.append((OP_STORE, 0))
            with np.errstate(all="ignore"):
                value = float(np.asarray(_run(sub_ops, sub_consts, 1, np.zeros((3, 1)), np.zeros((3, 1)))[0][0]).reshape(-1)[0])
        bits = np.float64(value).tobytes()
        for k in range(n_params, len(consts)):
            if np.float64(consts[k]).tobytes() == bits:
                break
        else:
            k = len(consts)
            consts.append(value)
        ops.append((OP_CONST, k))
        return
    _emit_plain(n, ops, consts, n_params)


def _emit_plain(n: _Node, ops: list, consts: list, n_params: int):
    if n.op == OP_CONST:
        consts.append(n.value)
        ops.append((OP_CONST, len(consts) - 1))
    elif n.op == _PARAM:
        ops.append((OP_CONST, n.value))
    elif n.op == _FIELD:
        ops.append((OP_X, 3 + n.value))
    elif n.op == _STATE:
        ops.append((OP_X, n.value))  # (name, k): Criterion.program(t, n_comp) writes the index
    elif n.op in (OP_X, OP_Y):
        ops.append((n.op, n.value))
    elif n.op == _POW:
        if n.power == 0:  # a**0 is 1 whatever a is
            _emit(_Node(OP_CONST, value=1.0), ops, consts, n_params)
            return
        _emit(n.args[0], ops, consts, n_params)
        ops.extend([(OP_DUP, 0)] * (n.power - 1))  # a a ... a, then the products: ((a a) a) a up to the order of commuting factors
        ops.extend([(OP_MUL, 0)] * (n.power - 1))
    else:
        for a in n.args:
            _emit(a, ops, consts, n_params)
        ops.append((n.op, 0))


def stack_depths(ops) -> list[int]:
    """Stack depth after every instruction (raises ValueError on an underflow): the simulation the library's validation runs."""
    depth, out = 0, []
    for op, _ in ops:
        pops = _POPS.get(op, 2)
        if depth < pops:
            raise ValueError("program: stack underflow")
        depth += _PUSHES.get(op, 1) - pops
        out.append(depth)
    return out


_ONE, _ZERO, _TWO = np.float64(1.0), np.float64(0.0), np.float64(2.0)


def _flag(m):
    return np.where(m, _ONE, _ZERO)


def _unary(op, a):
    """The value of a one-operand instruction."""
    if op == OP_NEG:
        return -a
    if op == OP_ABS:
        return np.abs(a)
    if op == OP_NOT:
        return _flag(a == 0.0)
    return _MATH_NUMPY[op](a)


def _binary(op, a, b):
    """The value of a two-operand instruction for (a, b), b on top."""
    if op == OP_ADD:
        return a + b
    if op == OP_SUB:
        return a - b
    if op == OP_MUL:
        return a * b
    if op == OP_DIV:
        return a / b
    if op == OP_MIN:
        return np.where(b < a, b, a)
    if op == OP_MAX:
        return np.where(b > a, b, a)
    if op == OP_LT:
        return _flag(a < b)
    if op == OP_LE:
        return _flag(a <= b)
    if op == OP_GT:
        return _flag(a > b)
    if op == OP_GE:
        return _flag(a >= b)
    if op == OP_AND:
        return _flag((a != 0.0) & (b != 0.0))
    if op == OP_OR:
        return _flag((a != 0.0) | (b != 0.0))
    raise ValueError(f"program: unknown opcode {op}")


# The tangent rules of include/hommx_hip.h (hommx_expand_tangents), as the kernel applies them: d_j of an instruction's result from the
# d_j of its operands -- p for the operand a of a one-operand instruction, (p, q) for (a, b), b on top; v: the instruction's value.  An
# instruction that is not here (a comparison, AND, OR, NOT) is piecewise constant
_TANGENT = {
    OP_NEG: lambda a, v, p: -p,
    OP_ABS: lambda a, v, p: np.where(a < 0.0, -p, p),
    OP_SQRT: lambda a, v, p: p / (_TWO * v),
    OP_SIN: lambda a, v, p: np.cos(a) * p,
    OP_COS: lambda a, v, p: -(np.sin(a) * p),
    OP_TAN: lambda a, v, p: p * (_ONE + v * v),
    OP_EXP: lambda a, v, p: v * p,
    OP_LOG: lambda a, v, p: p / a,
    OP_TANH: lambda a, v, p: p * (_ONE + -(v * v)),
    OP_ADD: lambda a, b, v, p, q: p + q,
    OP_SUB: lambda a, b, v, p, q: p + (-q),
    OP_MUL: lambda a, b, v, p, q: a * q + p * b,
    OP_DIV: lambda a, b, v, p, q: (p + -(v * q)) / b,
    OP_MIN: lambda a, b, v, p, q: np.where(b < a, q, p),
    OP_MAX: lambda a, b, v, p, q: np.where(b > a, q, p),
}


# The second-order rules of include/hommx_hip.h (hommx_expand_second_tangents), as the kernel applies them: h_ij of an instruction's
# result for the pair (i, j) of slots.  One operand (a, its tangents pi, pj, its ha): f(a, v, di, dj, pi, pj, ha); two, (a, pi, pj, ha)
# and (b, qi, qj, hb), b on top: f(a, b, v, di, dj, pi, pj, qi, qj, ha, hb).  v: the instruction's value, di, dj: its own tangents
# (``_TANGENT``).  An instruction that is not here is piecewise constant
_TANGENT2 = {
    OP_NEG: lambda a, v, di, dj, pi, pj, ha: -ha,
    OP_ABS: lambda a, v, di, dj, pi, pj, ha: np.where(a < 0.0, -ha, ha),
    OP_SQRT: lambda a, v, di, dj, pi, pj, ha: (ha + -((_TWO * di) * dj)) / (_TWO * v),
    OP_SIN: lambda a, v, di, dj, pi, pj, ha: np.cos(a) * ha + -((v * pi) * pj),
    OP_COS: lambda a, v, di, dj, pi, pj, ha: -(np.sin(a) * ha) + -((v * pi) * pj),
    OP_TAN: lambda a, v, di, dj, pi, pj, ha: (_ONE + v * v) * ha + ((_TWO * v) * dj) * pi,
    OP_EXP: lambda a, v, di, dj, pi, pj, ha: v * ha + dj * pi,
    OP_LOG: lambda a, v, di, dj, pi, pj, ha: (ha + -(pi * dj)) / a,
    OP_TANH: lambda a, v, di, dj, pi, pj, ha: (_ONE + -(v * v)) * ha + -(((_TWO * v) * dj) * pi),
    OP_ADD: lambda a, b, v, di, dj, pi, pj, qi, qj, ha, hb: ha + hb,
    OP_SUB: lambda a, b, v, di, dj, pi, pj, qi, qj, ha, hb: ha + (-hb),
    OP_MUL: lambda a, b, v, di, dj, pi, pj, qi, qj, ha, hb: ((a * hb + ha * b) + pi * qj) + pj * qi,
    OP_DIV: lambda a, b, v, di, dj, pi, pj, qi, qj, ha, hb: (((ha + -(di * qj)) + -(dj * qi)) + -(v * hb)) / b,
    OP_MIN: lambda a, b, v, di, dj, pi, pj, qi, qj, ha, hb: np.where(b < a, hb, ha),
    OP_MAX: lambda a, b, v, di, dj, pi, pj, qi, qj, ha, hb: np.where(b > a, hb, ha),
}


def _pairs(n: int) -> tuple:
    """The pairs (a, b), a <= b, of n slots in the row-major order of the ABI: (0,0), (0,1), .., (0,n-1), (1,1), ..."""
    return tuple((a, b) for a in range(n) for b in range(a, n))


def _run(ops, consts, n_comp: int, x, y, n_params: int = 0, n_fields: int = 0, second: bool = False, seeds=None) -> tuple:
    """Interpret a program with NumPy on x[3 + n_fields, ...] (the midpoint, then the fields: ``X k`` reads row k) and y[d, ...]
    (broadcast against each other), in forward mode over its P = n_params + n_fields differentiable slots, the parameters, then the
    fields (``CONST k``, k < n_params, seeds slot k; ``X k``, k >= 3, slot ``n_params + k - 3``): (values[n_comp],
    tangents[n_comp][P]), each operation the separately rounded IEEE operation k_expand_program<P> performs.  Like the kernel's, the
    value pass is the pass without slots: a stack entry is (v, [d_0 .. d_{P-1}]) and v is computed in one place whatever P is.

    A tangent that is None is +0.0 everywhere: where every operand's d_j is 0.0 the result's d_j is +0.0 and the formula is not
    evaluated -- structurally (None) or, point by point, through ``np.where`` -- so a sqrt(0) or a division by zero in a part of the
    expression that does not read slot j cannot make its tangent NaN.

    ``second``: the second-order pass, k_expand_program2 -- a stack entry is (v, [d_j], [h_ij for (i, j) in _pairs(P)]), v and d are
    computed by the same statements, and the result is (values, tangents, second[n_comp][n_pairs]).  Its dead rule: h_ij is +0.0
    (None) where every operand's h_ij is 0.0 and every operand's d_i, or every operand's d_j, is 0.0.

    ``seeds``: the rows of ``x`` that seed instead, as {row: slot} -- ``X row`` seeds slot ``seeds[row]``, every other read and every
    constant seeds nothing, and P = 1 + the largest slot (the forward mode of csrc/state_program.h over the strain rows)."""
    P = n_params + n_fields if seeds is None else 1 + max(seeds.values())
    if seeds is None:
        seed_const = lambda k, j: k == j and k < n_params
        seed_x = lambda k, j: k >= 3 and j == n_params + k - 3
    else:
        seed_const = lambda k, j: False
        seed_x = lambda k, j: seeds.get(k) == j
    pairs = _pairs(P) if second else ()
    stack, out_v, out_d, out_h = [], [None] * n_comp, [None] * n_comp, [None] * n_comp
    no_h = [None] * len(pairs)

    def zeros(ds):
        """Where every entry of ``ds`` (None: +0.0 everywhere) is 0.0."""
        full = [_ZERO if d is None else d for d in ds]
        dead = full[0] == 0.0
        for d in full[1:]:
            dead = dead & (d == 0.0)
        return dead

    def rule_h(formula, hs, dis, djs):
        """h_ij of a result from its operands' h_ij (hs) and tangents d_i (dis), d_j (djs): +0.0 where it is dead, else formula()."""
        if formula is None or (all(h is None for h in hs) and (all(d is None for d in dis) or all(d is None for d in djs))):
            return None
        return np.where(zeros(hs) & (zeros(dis) | zeros(djs)), _ZERO, formula())

    def fill(d):
        return _ZERO if d is None else d

    def rule(formula, *operands):
        """d_j of a result from the d_j of its operands: +0.0 where all of them are 0.0, else formula(*operands)."""
        if formula is None or all(d is None for d in operands):
            return None
        full = [_ZERO if d is None else d for d in operands]
        dead = full[0] == 0.0
        for d in full[1:]:
            dead = dead & (d == 0.0)
        return np.where(dead, _ZERO, formula(*full))

    for op, k in ops:
        if op == OP_CONST:
            stack.append((np.float64(consts[k]), [_ONE if seed_const(k, j) else None for j in range(P)], list(no_h)))
        elif op == OP_X:
            stack.append((np.asarray(x[k], dtype=np.float64), [_ONE if seed_x(k, j) else None for j in range(P)], list(no_h)))
        elif op == OP_Y:
            stack.append((np.asarray(y[k], dtype=np.float64), [None] * P, list(no_h)))
        elif op == OP_DUP:
            stack.append((stack[-1][0], list(stack[-1][1]), list(stack[-1][2])))
        elif op == OP_STORE:
            out_v[k], out_d[k], out_h[k] = stack.pop()
        elif op == OP_SELECT:
            (b, db, hb), (a, da, ha), (c, _, _) = stack.pop(), stack.pop(), stack.pop()  # a condition carries no tangent
            pick = c != 0.0
            stack.append((np.where(pick, a, b), [rule(lambda p, q: np.where(pick, p, q), da[j], db[j]) for j in range(P)],
                          [rule_h(lambda s=s: np.where(pick, fill(ha[s]), fill(hb[s])), [ha[s], hb[s]], [da[i], db[i]], [da[j], db[j]])
                           for s, (i, j) in enumerate(pairs)]))
        elif _POPS.get(op, 2) == 1:
            a, da, ha = stack.pop()
            v, f, g = _unary(op, a), _TANGENT.get(op), _TANGENT2.get(op)
            d = [rule(f and (lambda p: f(a, v, p)), da[j]) for j in range(P)]
            stack.append((v, d, [rule_h(g and (lambda s=s, i=i, j=j: g(a, v, fill(d[i]), fill(d[j]), fill(da[i]), fill(da[j]), fill(ha[s]))),
                                        [ha[s]], [da[i]], [da[j]]) for s, (i, j) in enumerate(pairs)]))
        else:
            (b, db, hb), (a, da, ha) = stack.pop(), stack.pop()
            v, f, g = _binary(op, a, b), _TANGENT.get(op), _TANGENT2.get(op)
            d = [rule(f and (lambda p, q: f(a, b, v, p, q)), da[j], db[j]) for j in range(P)]
            stack.append((v, d, [rule_h(g and (lambda s=s, i=i, j=j: g(a, b, v, fill(d[i]), fill(d[j]), fill(da[i]), fill(da[j]), fill(db[i]),
                                                                        fill(db[j]), fill(ha[s]), fill(hb[s]))),
                                        [ha[s], hb[s]], [da[i], db[i]], [da[j], db[j]]) for s, (i, j) in enumerate(pairs)]))
    return (out_v, out_d, out_h) if second else (out_v, out_d)


class Expression:
    """A coefficient ``A(x, y)`` given as text (module docstring: the grammar).

    ``Expression(text)`` is a scalar coefficient (the Poisson classes), ``Expression(lam=..., mu=...)`` a ``Lame`` pair (the elasticity
    classes), ``Expression([[a, b], [b, c]])`` a symmetric d x d matrix (the Poisson classes; the two texts of an off-diagonal entry must
    parse to equal trees).  ``Expression(["c0", "c1", ...])``, a FLAT list of 1 to 6 texts, is a vector (``shape == "vector"``): no
    coefficient but a load -- a polarisation or an eigenstrain of the solver classes (``set_polarisation`` / ``set_eigenstrain``), whose
    components stand in the order of the reconstruction's flux / strain; as a callable it returns ``[n_comp, ...]``, and its streams keep
    the component axis whatever its length.  Passing a coefficient as ``A`` lets the solver classes sample on the DEVICE: the points of the micro quadrature rule go
    once, three numbers per macro cell (its midpoint) after them, and a bytecode kernel forms the element means.

    ``degree``: the quadrature degree of the expression, estimated from its tree by UFL's rules -- a literal, ``x[i]``, ``p[k]`` and
    ``pi`` 0; ``y[i]`` 1; a sum or difference the larger; a product or quotient the sum; ``a**k`` k times; ``abs`` keeps; ``where`` /
    ``min`` / ``max`` the larger of the values (not the condition); a math function 0 of an argument of degree 0, else the argument's
    + 2.  (UFL is not installed where this is developed: the rules are recalled, not run.)  Several components: the largest.

    ``p=[...]``: the values of up to 4 parameters ``p[k]`` of the text, shared by all macro cells (a graded parameter is written
    ``p[0] + p[1]*x[0]``), ``parameter_names`` their names (default ``"p0"``, ``"p1"``, ...).  They are the first ``n_params``
    constants of the program, each in a slot of its own even when the text does not read it, and a subtree that reads one is never
    folded.  ``with_parameters(p)`` changes the values without parsing again.  ``p_degree``: the degree of the tree in the parameters,
    computed like ``degree`` -- ``p[k]`` 1; a literal, ``x``, ``y`` 0; ``+ - where min max`` the larger; ``*`` the sum; ``**k`` k times;
    ``/`` by something without parameters keeps; a quotient by, a math function of, or ``abs`` / ``min`` / ``max`` of something that
    reads a parameter: infinity.  ``affine_in_parameters``: ``p_degree <= 1``; the second derivatives along the parameter tangents
    are then the whole Hessian.  A parameter inside a comparison logs one WARNING: the derivative ignores the motion of the interface
    (it is zero almost everywhere); a smooth transition such as ``tanh`` is the way to differentiate a radius.

    ``pairs``: the pairs (a, b), a <= b, of the differentiable slots in the order of the second-order streams
    (``host_second_tangents``, hommx_expand_second_tangents): (0, 0), (0, 1), .., (1, 1), ...

    ``fields=2`` or ``fields=("radius", "phase")``: up to 4 fields ``f[k]`` (literal index), each ONE VALUE PER MACRO CELL -- a design
    variable, the macro solution at the midpoint, a random draw --, ``field_names`` their names (default ``"f0"``, ``"f1"``, ...).  The
    solver classes take the values with ``set_fields``; the device reads them from the cell's row, after the midpoint.  ``f[k]`` has
    quadrature degree 0 and ``p_degree`` 1, so ``p_degree`` and ``affine_in_parameters`` speak of parameters and fields together, and a
    field inside a comparison logs the same WARNING.  In this module the fields ride as extra rows of ``x``: ``components``,
    ``__call__``, ``host_stream`` and ``host_tangents`` take ``x`` with ``3 + n_fields`` entries, and ``host_tangents`` returns the
    ``n_params + n_fields`` differentiable slots, the parameters first.

    The object is also a plain callable ``A(x, y)`` -- it interprets ``program()`` with NumPy --, so every generic path accepts it.
    ``host_stream`` is the documented host equivalent of the device sampler, ``host_tangents`` of its forward-mode pass and
    ``host_second_tangents`` of its second-order pass: the same IEEE operations in the same order.
    """

    def __init__(self, text=None, *, lam=None, mu=None, p=None, parameter_names=None, fields=None):
        if (lam is None) != (mu is None) or (text is None) == (lam is None):
            raise ValueError("Expression(text), Expression([[a, b], [b, c]]), Expression([c0, c1, ...]) or Expression(lam=..., mu=...)")
        self.dim = None  # the d of a matrix
        values = _parameter_values(p, None) if p is not None else np.zeros(0)
        self.n_params = int(values.size)
        if parameter_names is None:
            parameter_names = tuple(f"p{k}" for k in range(self.n_params))
        self.parameter_names = tuple(str(s) for s in parameter_names)
        if len(self.parameter_names) != self.n_params:
            raise ValueError(f"expression: {len(self.parameter_names)} parameter_names for {self.n_params} parameters")
        self.n_fields, self.field_names = _field_names(fields)
        ctx = _Context(self.n_params if p is not None else None, self.n_fields if fields is not None else None)
        if lam is not None:
            self.shape, texts = "lame", [lam, mu]
        elif isinstance(text, (list, tuple)) and not any(isinstance(r, (list, tuple)) for r in text):
            if not 1 <= len(text) <= MAX_COMP:
                raise ValueError(f"expression: a vector has 1 .. {MAX_COMP} components; got {len(text)}")
            self.shape, texts = "vector", list(text)
        elif isinstance(text, (list, tuple)):
            d = len(text)
            if d not in (2, 3) or any(not isinstance(r, (list, tuple)) or len(r) != d for r in text):
                raise ValueError("expression: a matrix is 2 x 2 or 3 x 3 (nested lists; a flat list of texts is a vector)")
            self.shape, self.dim = "matrix", d
            pairs = [(0, 0), (1, 1), (0, 1)] if d == 2 else [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]  # the component order of the ABI
            for i, j in pairs:
                if i != j and _parse(text[i][j], _Context(ctx.n_params, ctx.n_fields)).key() != \
                        _parse(text[j][i], _Context(ctx.n_params, ctx.n_fields)).key():
                    raise ValueError(f"expression: the matrix must be symmetric; entries [{i}][{j}] and [{j}][{i}] differ")
            texts, self._pairs = [text[i][j] for i, j in pairs], pairs
        else:
            self.shape, texts = "scalar", [text]
        self.texts = tuple(str(t) for t in texts)
        trees = [_parse(t, ctx) for t in texts]
        self.n_comp = len(trees)
        self.degree = max(t.degree for t in trees)
        self.p_degree = max(t.p_degree for t in trees)
        self.affine_in_parameters = self.p_degree <= 1
        ops, consts = [], [float(v) for v in values]
        for c, t in enumerate(trees):
            _emit(t, ops, consts, self.n_params)
            ops.append((OP_STORE, c))
        if len(ops) > MAX_OPS:
            raise ValueError(f"expression: too long: {len(ops)} instructions, at most {MAX_OPS}")
        if len(consts) > MAX_CONSTS:
            raise ValueError(f"expression: too many constants: {len(consts)} (the parameters among them), at most {MAX_CONSTS}")
        deepest = max(stack_depths(ops))
        if deepest > MAX_STACK:
            raise ValueError(f"expression: too deep: stack depth {deepest}, at most {MAX_STACK}")
        self._ops = np.array(ops, dtype=np.uint8).reshape(-1, 2)
        self._consts = np.array(consts, dtype=np.float64)
        self.n_y = 1 + max([int(k) for op, k in ops if op == OP_Y], default=-1)  # fast-variable components the expression reads
        if ctx.compared:
            logging.getLogger(__name__).warning(
                "expression: a parameter occurs inside a comparison (%s): the derivative with respect to it ignores the motion of the "
                "interface (it is zero almost everywhere); use a smooth transition such as tanh to differentiate a radius",
                "; ".join(dict.fromkeys(ctx.compared)))

    @property
    def p(self) -> np.ndarray:
        """The values of the parameters (a copy)."""
        return self._consts[:self.n_params].copy()

    @property
    def pairs(self) -> tuple:
        """The pairs (a, b), a <= b, of the n_params + n_fields differentiable slots, in the order of the second-order streams."""
        return _pairs(self.n_params + self.n_fields)

    @property
    def _flat(self) -> bool:
        """Whether the streams drop the component axis: one component, except of a vector, which keeps its axis whatever its length."""
        return self.n_comp == 1 and self.shape != "vector"

    def with_parameters(self, p) -> "Expression":
        """The same expression at other parameter values: the same ``ops``, only ``consts[:n_params]`` replaced -- nothing is parsed."""
        values = _parameter_values(p, self.n_params)
        other = copy.copy(self)
        other._consts = self._consts.copy()
        other._consts[:self.n_params] = values
        return other

    def program(self) -> tuple[np.ndarray, np.ndarray]:
        """(ops[n_ops, 2] uint8 = (opcode, operand), consts[n_consts] float64): the postfix program of hommx_coef_program -- every
        component's code followed by its ``STORE c``.  The first ``n_params`` constants are the parameters."""
        return self._ops.copy(), self._consts.copy()

    def components(self, x, y) -> list:
        """The components at x[3 + n_fields, ...] (the midpoint, then the fields), y[d, ...], each broadcast to the common shape of x[0]
        and y[0]."""
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        self._check_rows(x.shape[0])
        if self.n_y > y.shape[0]:
            raise ValueError(f"the expression reads y[{self.n_y - 1}]; the fast variable has {y.shape[0]} components")
        shape = np.broadcast(x[0], y[0]).shape
        with np.errstate(all="ignore"):
            out, _ = _run(self._ops.tolist(), self._consts, self.n_comp, x, y)
        return [np.broadcast_to(v, shape) for v in out]

    def _check_rows(self, rows: int):
        if self.n_fields and rows < 3 + self.n_fields:
            raise ValueError(f"the expression reads the fields {', '.join(self.field_names)}: x must have 3 + {self.n_fields} entries "
                             f"(the midpoint, then the fields of the cell); got {rows}")

    def _rows(self, x) -> np.ndarray:
        """x as float64[N, 3 + n_fields]: the rows of the cells."""
        x = np.asarray(x, dtype=np.float64)
        if x.ndim >= 1:
            self._check_rows(x.shape[-1])
        return x.reshape(-1, 3 + self.n_fields)

    def __call__(self, x, y):
        v = self.components(x, y)
        if self.shape == "scalar":
            return np.array(v[0])
        if self.shape == "lame":
            from .hmm import Lame

            return Lame(np.array(v[0]), np.array(v[1]))
        if self.shape == "vector":
            return np.stack(v)
        out = np.empty(v[0].shape + (self.dim, self.dim))
        for c, (i, j) in enumerate(self._pairs):
            out[..., i, j] = out[..., j, i] = v[c]
        return out

    def host_stream(self, x: np.ndarray, yq: np.ndarray, w: np.ndarray) -> np.ndarray:
        """Element means coef[N, n_el(, n_comp)] at the rows x[N, 3 + n_fields] (midpoint, then fields) from the points yq[n_el, n_q, d] and
        weights w[n_q], exactly as the device forms them: ``acc = acc + w[q] * v_q`` with q ascending, from 0."""
        x = self._rows(x)
        n_el, nq, d = yq.shape
        acc = [np.zeros((x.shape[0], n_el)) for _ in range(self.n_comp)]
        for q in range(nq):
            v = self.components(x.T[:, :, None], np.moveaxis(yq[:, q, :], -1, 0)[:, None, :])
            for c in range(self.n_comp):
                acc[c] = acc[c] + w[q] * v[c]
        return acc[0] if self._flat else np.stack(acc, axis=-1)

    def host_tangents(self, x: np.ndarray, yq: np.ndarray, w: np.ndarray) -> np.ndarray:
        """The derivatives of ``host_stream`` with respect to the parameters, then the fields (of a cell: its own value),
        dirs[N, n_params + n_fields, n_el(, n_comp)], exactly as the device's forward-mode pass forms them (``_TANGENT``: the rules),
        ``acc_j = acc_j + w[q] * d_j`` with q ascending, from 0."""
        if self.n_params + self.n_fields == 0:
            raise ValueError("the expression has no parameters (p=[...])")
        x = self._rows(x)
        n_el, nq, d = yq.shape
        if self.n_y > d:
            raise ValueError(f"the expression reads y[{self.n_y - 1}]; the fast variable has {d} components")
        P, shape = self.n_params + self.n_fields, (x.shape[0], n_el)
        acc = [[np.zeros(shape) for _ in range(self.n_comp)] for _ in range(P)]
        ops = self._ops.tolist()
        for q in range(nq):
            with np.errstate(all="ignore"):
                _, dv = _run(ops, self._consts, self.n_comp, x.T[:, :, None], np.moveaxis(yq[:, q, :], -1, 0)[:, None, :], self.n_params,
                             self.n_fields)
            for j in range(P):
                for c in range(self.n_comp):
                    dj = np.float64(0.0) if dv[c][j] is None else dv[c][j]
                    acc[j][c] = acc[j][c] + w[q] * np.broadcast_to(dj, shape)
        out = np.stack([np.stack(a, axis=-1) for a in acc], axis=1)  # [N, P, n_el, n_comp]
        return out[..., 0] if self._flat else out


    def host_second_tangents(self, x: np.ndarray, yq: np.ndarray, w: np.ndarray) -> np.ndarray:
        """The second derivatives of ``host_stream`` with respect to the pairs ``self.pairs`` of the parameters, then the fields,
        curv[N, n_pairs, n_el(, n_comp)], exactly as the device's second-order forward-mode pass forms them (``_TANGENT2``: the rules),
        ``acc_ab = acc_ab + w[q] * h_ab`` with q ascending, from 0."""
        if self.n_params + self.n_fields == 0:
            raise ValueError("the expression has no parameters (p=[...])")
        x = self._rows(x)
        n_el, nq, d = yq.shape
        if self.n_y > d:
            raise ValueError(f"the expression reads y[{self.n_y - 1}]; the fast variable has {d} components")
        pairs, shape = self.pairs, (x.shape[0], n_el)
        acc = [[np.zeros(shape) for _ in range(self.n_comp)] for _ in pairs]
        ops = self._ops.tolist()
        for q in range(nq):
            with np.errstate(all="ignore"):
                _, _, hv = _run(ops, self._consts, self.n_comp, x.T[:, :, None], np.moveaxis(yq[:, q, :], -1, 0)[:, None, :], self.n_params,
                                self.n_fields, second=True)
            for s in range(len(pairs)):
                for c in range(self.n_comp):
                    hs = np.float64(0.0) if hv[c][s] is None else hv[c][s]
                    acc[s][c] = acc[s][c] + w[q] * np.broadcast_to(hs, shape)
        out = np.stack([np.stack(a, axis=-1) for a in acc], axis=1)  # [N, n_pairs, n_el, n_comp]
        return out[..., 0] if self._flat else out


class Criterion:
    """A failure criterion: ONE scalar expression of the reconstructed micro state of an element, evaluated on the device where the
    stress is formed (include/hommx_hip.h, hommx_criterion_source; csrc/criterion.hip) and, by ``host_values``, with
    NumPy -- the same operations in the same order.

    The grammar is ``Expression``'s with three more indexed names: ``s[k]``, k < t, the flux / stress of the element in the
    component order of ``Reconstruction.flux`` (shear not doubled); ``e[k]``, k < t, its gradient / strain in the order of
    ``Reconstruction.strain`` (shear doubled); ``c[k]``, k < n_comp, its coefficient entry (``c[0]`` of scalar Poisson, ``c[0],
    c[1]`` = lambda, mu, ...), so ``where(c[1] > 20, 900, 60)`` tells fibre from matrix whatever the form of the coefficient.
    ``x[i]`` is the macro midpoint, ``y[i]`` the fast variable AT THE ELEMENT CENTROID, ``p[k]`` the parameters (``p=[...]``,
    ``with_parameters``), ``f[k]`` per-cell fields of the criterion's own (``fields=``), a strength per macro cell, say.

    No opcode is added: the state is read like a field, through ``X k`` on a wider row -- ``e[k]`` is ``X 3 + n_fields + k``,
    ``s[k]`` ``X 3 + n_fields + t + k`` and ``c[k]`` ``X 3 + n_fields + 2 t + k``.  t and n_comp are the plan's, so the program is
    written, and the indices are checked, when the criterion meets one: ``program(t, n_comp)``.  The limits of a program hold (128
    instructions, 32 constants with the parameters first, depth 16), and it has one component.

    ``threshold``: the value from which an element counts into ``CriterionResult.exceed_volume`` (default 1: an index).

    A criterion of the NONLINEAR state (the tail of ``MicroCellPlan.secant``, ``criterion(nonlinear=True)`` of the solver
    classes) reads two more names: ``b[k]``, k < n_comp, the BASE coefficient of the element -- what the solver's ``A`` gives and a
    ``SecantLaw`` calls ``c[k]``; ``c[k]`` stays the coefficient the stress was formed with, the softened one --, and, with
    ``history=n``, ``h[k]``, k < n, the history variable of the element at the start of the load step, the value the law's ``h[k]``
    reads.  The row is the law's with the base behind it, ``[midpoint 3 | fields | e (t) | s (t) | c (n_comp) | h (n_history) |
    b (n_comp)]``, so ``h[k]`` has the index it has in a ``SecantLaw``; a criterion that reads neither has the program it had.
    ``reads_state``: it reads ``b`` or ``h`` and can be evaluated on a nonlinear state only."""

    def __init__(self, text, p=None, parameter_names=None, fields=None, threshold=1.0, history=None):
        values = _parameter_values(p, None) if p is not None else np.zeros(0)
        self.n_params = int(values.size)
        if parameter_names is None:
            parameter_names = tuple(f"p{k}" for k in range(self.n_params))
        self.parameter_names = tuple(str(s) for s in parameter_names)
        if len(self.parameter_names) != self.n_params:
            raise ValueError(f"criterion: {len(self.parameter_names)} parameter_names for {self.n_params} parameters")
        self.n_fields, self.field_names = _field_names(fields)
        self.threshold = float(threshold)
        if math.isnan(self.threshold):
            raise ValueError("criterion: the threshold is NaN")
        if history is not None and (isinstance(history, bool) or not isinstance(history, int) or not 1 <= history <= MAX_HISTORY):
            raise ValueError(f"criterion: history is the number of history variables, 1 .. {MAX_HISTORY}; got {history!r}")
        self.n_history = 0 if history is None else int(history)
        self.text = str(text)
        tree = _parse(text, _Context(self.n_params if p is not None else None, self.n_fields if fields is not None else None, state=True,
                                     n_history=history, base=True))
        ops, consts = [], [float(v) for v in values]
        _emit(tree, ops, consts, self.n_params)
        ops.append((OP_STORE, 0))
        if len(ops) > MAX_OPS:
            raise ValueError(f"criterion: too long: {len(ops)} instructions, at most {MAX_OPS}")
        if len(consts) > MAX_CONSTS:
            raise ValueError(f"criterion: too many constants: {len(consts)} (the parameters among them), at most {MAX_CONSTS}")
        self.depth = max(stack_depths(ops))
        if self.depth > MAX_STACK:
            raise ValueError(f"criterion: too deep: stack depth {self.depth}, at most {MAX_STACK}")
        self._ops = ops  # the operand of a state read is still (name, k)
        self._consts = np.array(consts, dtype=np.float64)
        self.n_y = 1 + max([int(k) for op, k in ops if op == OP_Y], default=-1)  # fast-variable components the criterion reads
        self.state_indices = {name: 1 + max([k[1] for op, k in ops if op == OP_X and isinstance(k, tuple) and k[0] == name], default=-1)
                              for name in "escbh"}  # entries of e, s, c, b and h it reads
        self.reads_state = bool(self.state_indices["b"] or self.state_indices["h"])

    @property
    def p(self) -> np.ndarray:
        """The values of the parameters (a copy)."""
        return self._consts[:self.n_params].copy()

    def with_parameters(self, p) -> "Criterion":
        """The same criterion at other parameter values: only ``consts[:n_params]`` replaced -- nothing is parsed."""
        values = _parameter_values(p, self.n_params)
        other = copy.copy(self)
        other._consts = self._consts.copy()
        other._consts[:self.n_params] = values
        return other

    def program(self, t: int, n_comp: int, n_history: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """(ops[n_ops, 2] uint8, consts[n_consts] float64) on a plan of tensor size ``t`` whose coefficient has ``n_comp`` entries per
        element: the one component's code and ``STORE 0``.  ``h[k]`` is ``X 3 + n_fields + 2 t + n_comp + k`` and ``b[k]``
        ``X 3 + n_fields + 2 t + n_comp + n_history + k``.  ``n_history``: the history variables of the row the program runs on, the
        law's (default: the declared number); a criterion declared without ``history=`` runs on the row of any law, one declared
        with it on the row of a law with as many -- ``ValueError`` naming both numbers otherwise.  ``ValueError`` as well for an
        index of ``s`` / ``e`` at or above t, of ``c`` / ``b`` at or above n_comp."""
        if n_history is None:
            n_history = self.n_history
        if self.n_history and int(n_history) != self.n_history:
            raise ValueError(f"criterion: it declares history={self.n_history}; the law has {int(n_history)} history variables (declare "
                             f"Criterion(..., history={int(n_history) or None}))")
        base = {"e": 3 + self.n_fields, "s": 3 + self.n_fields + t, "c": 3 + self.n_fields + 2 * t,
                "h": 3 + self.n_fields + 2 * t + n_comp, "b": 3 + self.n_fields + 2 * t + n_comp + int(n_history)}
        for name, bound, what in (("e", t, "t"), ("s", t, "t"), ("c", n_comp, "n_comp"), ("b", n_comp, "n_comp")):
            if self.state_indices[name] > bound:
                raise ValueError(f"criterion: {name}[{self.state_indices[name] - 1}] is out of range: the plan has {what} = {bound} "
                                 f"(t = {t}, n_comp = {n_comp})")
        ops = [(op, base[k[0]] + k[1] if isinstance(k, tuple) else k) for op, k in self._ops]
        return np.array(ops, dtype=np.uint8).reshape(-1, 2), self._consts.copy()

    def host_values(self, e, s, c, x, y=None, fields=None, base=None, history=None) -> np.ndarray:
        """values[N, n_el]: the criterion of every element from e[N, n_el, t] and s[N, n_el, t] (``CriterionResult.strain`` / ``flux``),
        c[N, n_el(, n_comp)] (the coefficient stream), x[N, 3] (the macro midpoints), y[n_el, d] (the element centroids; may be None
        when the criterion reads no ``y``) and fields[N, n_fields] -- ``_run``, value pass, on the rows the device reads: the
        midpoint, the fields, then e, s and c of the element.  A state criterion: base[N, n_el(, n_comp)] is what ``b[k]`` reads
        and history[N, n_el, n_history] what ``h[k]`` reads, behind c on the row; ``ValueError`` when the criterion reads a name
        whose array is missing.  Bit for bit the device's values wherever the program holds exactly rounded operations only."""
        e, s = np.asarray(e, dtype=np.float64), np.asarray(s, dtype=np.float64)
        N, n_el, t = e.shape
        c = np.asarray(c, dtype=np.float64).reshape(N, n_el, -1)
        state = [e, s, c]
        if self.state_indices["h"] and history is None:
            raise ValueError(f"the criterion reads h[{self.state_indices['h'] - 1}]: pass history[N, n_el, {self.n_history}]")
        if history is not None:  # the row of the law the state belongs to: its history, read or not, stands between c and b
            history = np.asarray(history, dtype=np.float64)
            if history.ndim == 2:
                history = history[:, :, None]
            if history.ndim != 3 or history.shape[:2] != (N, n_el):
                raise ValueError(f"history must be [N, n_el, n_history] = [{N}, {n_el}, n_history]; got shape {history.shape}")
            state.append(history)
        ops, consts = self.program(t, c.shape[2], 0 if history is None else history.shape[2])
        if self.state_indices["b"]:
            if base is None:
                raise ValueError(f"the criterion reads b[{self.state_indices['b'] - 1}]: pass the base coefficient stream "
                                 f"base[N, n_el, {c.shape[2]}]")
            if np.size(base) != c.size:
                raise ValueError(f"base must have the shape of c, [{N}, {n_el}, {c.shape[2]}]; got shape {np.shape(base)}")
            state.append(np.asarray(base, dtype=np.float64).reshape(c.shape))
        x = np.asarray(x, dtype=np.float64).reshape(N, -1)
        x = np.concatenate([x, np.zeros((N, 3 - x.shape[1]))], axis=1) if x.shape[1] < 3 else x[:, :3]
        if self.n_fields:
            if fields is None:
                raise ValueError(f"the criterion reads the fields {', '.join(self.field_names)}: pass fields[N, {self.n_fields}]")
            fields = np.asarray(fields, dtype=np.float64).reshape(N, self.n_fields)
        if self.n_y and (y is None or np.shape(y)[-1] < self.n_y):
            raise ValueError(f"the criterion reads y[{self.n_y - 1}]: pass the element centroids y[n_el, d]")
        rows = [x[:, k, None] for k in range(3)] + [fields[:, k, None] for k in range(self.n_fields)]
        rows += [a[:, :, k] for a in state for k in range(a.shape[2])]
        yr = [] if y is None else [np.asarray(y, dtype=np.float64)[None, :, k] for k in range(np.shape(y)[-1])]
        with np.errstate(all="ignore"):
            out, _ = _run(ops.tolist(), consts, 1, rows, yr)
        return np.array(np.broadcast_to(out[0], (N, n_el)))

    # -- ready-made texts ------------------------------------------------------------------------------------------------------------
    @classmethod
    def flux_norm(cls, kind: str, dim: int, **kw) -> "Criterion":
        """The norm ``reconstruct`` reports as ``max_flux``: |q| for the Poisson kinds, the Frobenius norm of the stress tensor (shear
        entries counted twice) for the elasticity kinds -- ``sqrt(sum_k w_k s[k]**2)``."""
        elastic = kind.startswith("elasticity")
        t = dim * (dim + 1) // 2 if elastic else dim
        terms = [("2*" if elastic and k >= dim else "") + f"s[{k}]**2" for k in range(t)]
        return cls("sqrt(" + " + ".join(terms) + ")", **kw)

    @classmethod
    def von_mises(cls, dim: int, strength="1", plane: str = "strain", **kw) -> "Criterion":
        """The von Mises stress over ``strength`` (any text of the grammar: it may read ``c``, ``y``, ``x``, ``p`` and ``f``) for the
        ``Lame`` kinds.  2D, ``plane="strain"``: the out-of-plane stress is ``c[0]*(e[0] + e[1])``; ``plane="stress"``: it is 0."""
        if plane not in ("strain", "stress"):
            raise ValueError(f"plane must be 'strain' or 'stress'; got {plane!r}")
        if dim == 3:
            a, b, c3, shear = "s[0]", "s[1]", "s[2]", "s[3]**2 + s[4]**2 + s[5]**2"
        elif dim == 2:
            a, b, c3, shear = "s[0]", "s[1]", "(c[0]*(e[0] + e[1]))" if plane == "strain" else "0.0", "s[2]**2"
        else:
            raise ValueError(f"dim must be 2 or 3; got {dim}")
        return cls(f"sqrt(0.5*(({a} - {b})**2 + ({b} - {c3})**2 + ({c3} - {a})**2) + 3*({shear})) / ({strength})", **kw)

    @classmethod
    def max_principal(cls, strength="1", **kw) -> "Criterion":
        """The largest principal stress of 2D elasticity over ``strength``."""
        return cls(f"(0.5*(s[0] + s[1]) + sqrt((0.5*(s[0] - s[1]))**2 + s[2]**2)) / ({strength})", **kw)


class SecantLaw:
    """A strain-dependent coefficient: the entries of an element's coefficient as expressions of its own micro state, iterated on the
    device as a secant (Kacanov) iteration (include/hommx_hip.h, hommx_secant_source; csrc/secant.hip) and, by
    ``host_values``, evaluated with NumPy -- the same operations in the same order.

    The component shapes are ``Expression``'s: ``SecantLaw(text)`` one component (scalar Poisson), ``SecantLaw([[a, b], [b, c]])`` a
    symmetric d x d matrix in the ``poisson_matrix`` order of the ABI, ``SecantLaw(lam=..., mu=...)`` the two Lame entries, and a
    FLAT list of ``n_comp`` texts the Voigt kind (6 entries in 2D, 21 in 3D).  The grammar is ``Criterion``'s: a law reads

    * ``c[k]``: the BASE coefficient of the element -- what the solver's coefficient ``A`` gives --, so ``where(c[0] > 5, c[0], ...)``
      tells the phases apart;
    * ``e[k]``: the gradient / strain of the current iterate (shear doubled);
    * ``s[k]`` = material(current coefficient) e: the secant flux / stress of the current iterate;
    * ``x[i]``, ``y[i]`` (the element centroid), ``p[k]`` and ``f[k]`` as a ``Criterion`` does.

    No opcode is added: ``program(t, n_comp)`` is on the row of a criterion, ``[midpoint 3 | fields | e (t) | s (t) | c (n_comp)]``,
    with one ``STORE k`` per component.  The limits of a program hold for all components together (128 instructions, 32 constants
    with the parameters first, depth 16), and the number of components must be the plan's ``n_comp``.

    The iteration converges when s -> s a(s) is increasing (a monotone law).  ``explicit``: the law reads no ``s[k]``; such a law has
    a consistent tangent d sigma_H / d xi at its converged state (``host_tangent`` is the NumPy twin of the device's
    tangent coefficient), which ``MicroCellPlan.secant_tangent`` and ``solve_nonlinear(method="newton")`` use.  The tangent of an
    implicit law (one that reads ``s``) is out of scope.

    History variables: ``history=[text_0, ...]`` gives the law 1 .. ``MAX_HISTORY`` internal variables per micro
    element, named ``history_names`` (default ``h0, h1, ...``) and starting from ``history_initial`` (a scalar or one value per
    variable).  ``h[k]`` is then a state name of every component text and every update text: the element's value at the START of the
    call, frozen for the whole iteration.  ``history[i]`` is the update, the new value of ``h[i]`` at the state of a round; what the
    stopping round gives is the call's ``history`` output, and the caller decides when it becomes the state (``commit_history`` of
    the solver classes).  The row grows by the history, ``[... | c (n_comp) | h (n_history)]``, and the update code stands behind
    the component code with ``STORE n_comp + i``; the limits hold for everything together.  ``explicit`` counts the updates too; the
    tangent differentiates the components only, on the program truncated behind the last component's ``STORE`` (``n_law_ops``)."""

    def __init__(self, text=None, *, lam=None, mu=None, p=None, parameter_names=None, fields=None, history=None, history_names=None,
                 history_initial=0.0):
        if (lam is None) != (mu is None) or (text is None) == (lam is None):
            raise ValueError("SecantLaw(text), SecantLaw([[a, b], [b, c]]), SecantLaw([c0, c1, ...]) or SecantLaw(lam=..., mu=...)")
        if history is None:
            if history_names is not None:
                raise ValueError("law: history_names without history=[...]")
            updates = []
        else:
            updates = [history] if isinstance(history, (str, int, float)) and not isinstance(history, bool) else list(history)
            if not 1 <= len(updates) <= MAX_HISTORY:
                raise ValueError(f"law: history has 1 .. {MAX_HISTORY} update texts; got {len(updates)}")
        self.n_history = len(updates)
        if history_names is None:
            history_names = tuple(f"h{k}" for k in range(self.n_history))
        self.history_names = tuple(str(s) for s in history_names)
        if len(self.history_names) != self.n_history:
            raise ValueError(f"law: {len(self.history_names)} history_names for {self.n_history} history variables")
        try:
            initial = np.array(history_initial, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            initial = np.zeros(0)
        if initial.size not in (1, self.n_history) or not np.all(np.isfinite(initial)):
            raise ValueError(f"law: history_initial is one finite number or one per history variable ({self.n_history}); got {history_initial!r}")
        self.history_initial = np.broadcast_to(initial, (self.n_history,)).copy()
        values = _parameter_values(p, None) if p is not None else np.zeros(0)
        self.n_params = int(values.size)
        if parameter_names is None:
            parameter_names = tuple(f"p{k}" for k in range(self.n_params))
        self.parameter_names = tuple(str(s) for s in parameter_names)
        if len(self.parameter_names) != self.n_params:
            raise ValueError(f"law: {len(self.parameter_names)} parameter_names for {self.n_params} parameters")
        self.n_fields, self.field_names = _field_names(fields)
        self.dim = None  # the d of a matrix
        ctx = lambda: _Context(self.n_params if p is not None else None, self.n_fields if fields is not None else None, state=True,
                               n_history=self.n_history if history is not None else None)
        if lam is not None:
            self.shape, texts = "lame", [lam, mu]
        elif isinstance(text, (list, tuple)) and not any(isinstance(r, (list, tuple)) for r in text):
            if not 1 <= len(text) <= MAX_LAW_COMP:
                raise ValueError(f"law: a flat list has 1 .. {MAX_LAW_COMP} components; got {len(text)}")
            self.shape, texts = "vector", list(text)
        elif isinstance(text, (list, tuple)):
            d = len(text)
            if d not in (2, 3) or any(not isinstance(r, (list, tuple)) or len(r) != d for r in text):
                raise ValueError("law: a matrix is 2 x 2 or 3 x 3 (nested lists; a flat list of texts is the Voigt kind)")
            self.shape, self.dim = "matrix", d
            pairs = [(0, 0), (1, 1), (0, 1)] if d == 2 else [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]  # the component order of the ABI
            for i, j in pairs:
                if i != j and _parse(text[i][j], ctx()).key() != _parse(text[j][i], ctx()).key():
                    raise ValueError(f"law: the matrix must be symmetric; entries [{i}][{j}] and [{j}][{i}] differ")
            texts = [text[i][j] for i, j in pairs]
        else:
            self.shape, texts = "scalar", [text]
        self.texts = tuple(str(t) for t in texts)
        self.n_comp = len(texts)
        ops, consts = [], [float(v) for v in values]
        for c, t in enumerate(texts):
            _emit(_parse(t, ctx()), ops, consts, self.n_params)
            ops.append((OP_STORE, c))
        self.n_law_ops = len(ops)  # the program of the tangent pass: the components alone
        self.history_texts = tuple(str(t) for t in updates)
        for i, t in enumerate(updates):
            _emit(_parse(t, ctx()), ops, consts, self.n_params)
            ops.append((OP_STORE, self.n_comp + i))
        if len(ops) > MAX_OPS:
            raise ValueError(f"law: too long: {len(ops)} instructions, at most {MAX_OPS}")
        if len(consts) > MAX_CONSTS:
            raise ValueError(f"law: too many constants: {len(consts)} (the parameters among them), at most {MAX_CONSTS}")
        self.depth = max(stack_depths(ops))
        if self.depth > MAX_STACK:
            raise ValueError(f"law: too deep: stack depth {self.depth}, at most {MAX_STACK}")
        self._ops = ops  # the operand of a state read is still (name, k)
        self._consts = np.array(consts, dtype=np.float64)
        self.n_y = 1 + max([int(k) for op, k in ops if op == OP_Y], default=-1)  # fast-variable components the law reads
        self.state_indices = {name: 1 + max([k[1] for op, k in ops if op == OP_X and isinstance(k, tuple) and k[0] == name], default=-1)
                              for name in ("esch" if self.n_history else "esc")}  # entries of e, s, c (and h, of a law with history) it reads

    @property
    def p(self) -> np.ndarray:
        """The values of the parameters (a copy)."""
        return self._consts[:self.n_params].copy()

    def with_parameters(self, p) -> "SecantLaw":
        """The same law at other parameter values: only ``consts[:n_params]`` replaced -- nothing is parsed."""
        values = _parameter_values(p, self.n_params)
        other = copy.copy(self)
        other._consts = self._consts.copy()
        other._consts[:self.n_params] = values
        return other

    def program(self, t: int, n_comp: int) -> tuple[np.ndarray, np.ndarray]:
        """(ops[n_ops, 2] uint8, consts[n_consts] float64) on a plan of tensor size ``t`` whose coefficient has ``n_comp`` entries per
        element: every component's code followed by its ``STORE k``, then every history update's followed by its ``STORE n_comp + i``;
        ``h[k]`` is ``X 3 + n_fields + 2 t + n_comp + k``.  ``ValueError`` when the law has another number of components than
        ``n_comp`` (naming both), for an index of ``s`` / ``e`` at or above t, of ``c`` at or above n_comp."""
        if self.n_comp != n_comp:
            raise ValueError(f"law: it has {self.n_comp} components; the plan's coefficient has n_comp = {n_comp}")
        base = {"e": 3 + self.n_fields, "s": 3 + self.n_fields + t, "c": 3 + self.n_fields + 2 * t, "h": 3 + self.n_fields + 2 * t + n_comp}
        for name, bound, what in (("e", t, "t"), ("s", t, "t"), ("c", n_comp, "n_comp")):
            if self.state_indices[name] > bound:
                raise ValueError(f"law: {name}[{self.state_indices[name] - 1}] is out of range: the plan has {what} = {bound} "
                                 f"(t = {t}, n_comp = {n_comp})")
        ops = [(op, base[k[0]] + k[1] if isinstance(k, tuple) else k) for op, k in self._ops]
        return np.array(ops, dtype=np.uint8).reshape(-1, 2), self._consts.copy()

    def _state_rows(self, e, s, c, x, y, fields, history) -> tuple:
        """(ops, consts, rows, y rows, N, n_el, t): the program on the plan the arrays belong to and the rows the device reads -- the
        midpoint, the fields, then e, s, c and the history of the element.  The checks of the three twins."""
        e, s = np.asarray(e, dtype=np.float64), np.asarray(s, dtype=np.float64)
        N, n_el, t = e.shape
        c = np.asarray(c, dtype=np.float64).reshape(N, n_el, -1)
        ops, consts = self.program(t, c.shape[2])
        x = np.asarray(x, dtype=np.float64).reshape(N, -1)
        x = np.concatenate([x, np.zeros((N, 3 - x.shape[1]))], axis=1) if x.shape[1] < 3 else x[:, :3]
        if self.n_fields:
            if fields is None:
                raise ValueError(f"the law reads the fields {', '.join(self.field_names)}: pass fields[N, {self.n_fields}]")
            fields = np.asarray(fields, dtype=np.float64).reshape(N, self.n_fields)
        if self.n_y and (y is None or np.shape(y)[-1] < self.n_y):
            raise ValueError(f"the law reads y[{self.n_y - 1}]: pass the element centroids y[n_el, d]")
        state = [e, s, c]
        if self.n_history:
            if history is None or np.size(history) != N * n_el * self.n_history:
                raise ValueError(f"the law has the history variables {', '.join(self.history_names)}: pass "
                                 f"history[N, n_el, {self.n_history}] = [{N}, {n_el}, {self.n_history}]")
            state.append(np.asarray(history, dtype=np.float64).reshape(N, n_el, self.n_history))
        elif history is not None:
            raise ValueError("the law has no history variables: history must be None")
        rows = [x[:, k, None] for k in range(3)] + [fields[:, k, None] for k in range(self.n_fields)]
        rows += [a[:, :, k] for a in state for k in range(a.shape[2])]
        yr = [] if y is None else [np.asarray(y, dtype=np.float64)[None, :, k] for k in range(np.shape(y)[-1])]
        return ops.tolist(), consts, rows, yr, N, n_el, t

    def host_values(self, e, s, c, x, y=None, fields=None, history=None) -> np.ndarray:
        """values[N, n_el, n_comp]: the law on every element from e[N, n_el, t] and s[N, n_el, t] (the strain and the secant flux of
        the current iterate), c[N, n_el(, n_comp)] (the BASE coefficient stream), x[N, 3] (the macro midpoints), y[n_el, d] (the
        element centroids; may be None when the law reads no ``y``), fields[N, n_fields] and, for a law with history variables,
        history[N, n_el, n_history] (what ``h[k]`` reads) -- ``_run``, value pass, on the rows the device reads.  Bit for bit the
        device's ``law_values`` wherever the program holds exactly rounded operations only."""
        ops, consts, rows, yr, N, n_el, _ = self._state_rows(e, s, c, x, y, fields, history)
        with np.errstate(all="ignore"):
            out, _ = _run(ops, consts, self.n_comp + self.n_history, rows, yr)
        return np.stack([np.array(np.broadcast_to(v, (N, n_el))) for v in out[:self.n_comp]], axis=-1)

    def host_history(self, e, s, c, x, y=None, fields=None, history=None) -> np.ndarray:
        """history_out[N, n_el, n_history]: the updates of the history variables on every element, from the arguments of
        ``host_values`` -- the same ``_run`` of the same program, its stores ``n_comp ..``.  Bit for bit the device's ``history``
        of a cell that stops in this state, wherever the program holds exactly rounded operations only."""
        if not self.n_history:
            raise ValueError("the law has no history variables (history=[...])")
        ops, consts, rows, yr, N, n_el, _ = self._state_rows(e, s, c, x, y, fields, history)
        with np.errstate(all="ignore"):
            out, _ = _run(ops, consts, self.n_comp + self.n_history, rows, yr)
        return np.stack([np.array(np.broadcast_to(v, (N, n_el))) for v in out[self.n_comp:]], axis=-1)

    @property
    def explicit(self) -> bool:
        """Whether the law reads no ``s[k]``: its coefficient is then a function of the strain, and it has a consistent tangent."""
        return self.state_indices["s"] == 0

    def _entries(self, t: int) -> list:
        """(r, c), r <= c, of every coefficient entry of a matrix (the ABI's order) or a Voigt law (upper triangle, row-major)."""
        if self.shape == "matrix":
            return [(0, 0), (1, 1), (0, 1)] if t == 2 else [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]
        return [(m, n) for m in range(t) for n in range(m, t)]

    def _material(self, c, t: int) -> np.ndarray:
        """C[..., t, t] = material(c[..., n_comp]) in the basis of the canonical loads, as csrc/mesh_elem.h forms it."""
        c = np.asarray(c, dtype=np.float64)
        C = np.zeros(c.shape[:-1] + (t, t))
        if self.shape == "scalar":
            for m in range(t):
                C[..., m, m] = c[..., 0]
        elif self.shape == "lame":
            dim = 2 if t == 3 else 3
            for m in range(t):
                for n in range(t):
                    C[..., m, n] = (c[..., 0] if m < dim and n < dim else 0.0) + ((2.0 * c[..., 1] if m < dim else c[..., 1]) if m == n else 0.0)
        else:
            for k, (r, q) in enumerate(self._entries(t)):
                C[..., r, q] = C[..., q, r] = c[..., k]
        return C

    def _material_columns(self, e) -> list:
        """g_k[..., t] = material(unit_k) e for every coefficient entry k, in the operation order of material_column (csrc/mesh_elem.h):
        copies of entries of e and +0.0, except the Lame pair -- lambda: (e0 + e1) (+ e2, added last) on the normal rows; mu: 2 e[m]
        on the normal rows, e[m] on the shear rows."""
        e = np.asarray(e, dtype=np.float64)
        t = e.shape[-1]
        if self.shape == "scalar":
            return [e.copy()]
        if self.shape == "lame":
            dim = 2 if t == 3 else 3
            tr = e[..., 0] + e[..., 1]
            if dim == 3:
                tr = tr + e[..., 2]
            g0, g1 = np.zeros_like(e), e.copy()
            for m in range(dim):
                g0[..., m] = tr
                g1[..., m] = 2.0 * e[..., m]
            return [g0, g1]
        out = []
        for r, q in self._entries(t):
            g = np.zeros_like(e)
            g[..., r] = e[..., q]
            g[..., q] = e[..., r]
            out.append(g)
        return out

    def host_tangent(self, e, cur, c, x, y=None, fields=None, history=None) -> tuple[np.ndarray, np.ndarray]:
        """(T_sym[N, n_el, t, t], asymmetry[N]): the coefficient of the consistent tangent as the device forms it (csrc/secant_tangent.hip;
        DESIGN 4.16) from e[N, n_el, t] (the strain of the stopping round), cur[N, n_el(, n_comp)] (the stream of that round,
        ``SecantResult.coef``), c (the BASE stream) and x, y, fields as ``host_values`` takes them.  ``_run`` in forward mode with the
        strain rows as seeds gives d_k[n] = dL_k/de[n]; then, in the order of the program's STOREs,
        ``T[m][n] = T[m][n] + g_k[m] * d_k[n]`` from ``material(cur)``, the symmetric part ``0.5 * (T[m][n] + T[n][m])`` and
        ``asymmetry = max |T - T^T| / max |T|`` per cell (0 when both are 0; a NaN never wins).  Bit for bit the device's
        ``tangent_coef`` wherever the program holds exactly rounded operations only.  ``ValueError`` for a law that reads ``s[k]``.
        ``history[N, n_el, n_history]``: what ``h[k]`` reads, for a law with history variables; the tangent differentiates the
        components at that frozen history (``max(h[0], ...)`` has the loading and the unloading branch), not the updates."""
        if not self.explicit:
            raise ValueError(f"law: it reads s[{self.state_indices['s'] - 1}]: the consistent tangent takes an explicit law, one that "
                             "reads no s[k]; an implicit law is out of scope")
        e = np.asarray(e, dtype=np.float64)
        ops, consts, rows, yr, N, n_el, t = self._state_rows(e, np.zeros_like(e), c, x, y, fields, history)
        ops = ops[:self.n_law_ops]  # the components alone: the updates stand behind the last component's STORE
        cur = np.asarray(cur, dtype=np.float64).reshape(N, n_el, -1)
        base = 3 + self.n_fields
        with np.errstate(all="ignore"):
            _, dv = _run(ops, consts, self.n_comp, rows, yr, seeds={base + n: n for n in range(t)})
            T = self._material(cur, t)
            g = self._material_columns(e)
            for k in [int(k) for op, k in ops if op == OP_STORE]:
                for n in range(t):
                    d = np.broadcast_to(np.float64(0.0) if dv[k][n] is None else dv[k][n], (N, n_el))
                    for m in range(t):
                        T[:, :, m, n] = T[:, :, m, n] + g[k][:, :, m] * d
            Tt = T.transpose(0, 1, 3, 2)
            skew = np.fmax.reduce(np.abs(T - Tt).reshape(N, -1), axis=1, initial=0.0)
            top = np.fmax.reduce(np.abs(T).reshape(N, -1), axis=1, initial=0.0)
            asym = np.where((skew == 0.0) & (top == 0.0), 0.0, skew / np.where(top == 0.0, 1.0, top))
        return 0.5 * (T + Tt), asym


def _field_names(fields) -> tuple[int, tuple]:
    """(n_fields, field_names) of ``fields=``: a count, or the names."""
    if fields is None:
        return 0, ()
    if isinstance(fields, (int, np.integer)) and not isinstance(fields, bool):
        names = tuple(f"f{k}" for k in range(int(fields)))
        if fields < 0:
            raise ValueError(f"expression: fields must be a count 0 .. {MAX_FIELDS} or a sequence of names; got {fields!r}")
    elif isinstance(fields, (list, tuple)) and all(isinstance(s, str) for s in fields):
        names = tuple(fields)
    else:
        raise ValueError(f"expression: fields must be a count 0 .. {MAX_FIELDS} or a sequence of names; got {fields!r}")
    if len(names) > MAX_FIELDS:
        raise ValueError(f"expression: at most {MAX_FIELDS} fields; got {len(names)}")
    return len(names), names


def _parameter_values(p, n_params: int | None) -> np.ndarray:
    """p as float64[n_params] (``n_params`` None: whatever its length, up to MAX_PARAMS), every value finite."""
    try:
        values = np.array(p, dtype=np.float64).reshape(-1) if np.ndim(p) <= 1 else None
    except (TypeError, ValueError):
        values = None
    if values is None:
        raise ValueError(f"expression: p must be a sequence of numbers; got {p!r}")
    if values.size > MAX_PARAMS:
        raise ValueError(f"expression: at most {MAX_PARAMS} parameters; got {values.size}")
    if n_params is not None and values.size != n_params:
        raise ValueError(f"expression: the expression has {n_params} parameters; got {values.size} values")
    for k, v in enumerate(values):
        if not np.isfinite(v):
            raise ValueError(f"expression: parameter p[{k}] is not finite: {v}")
    return values
