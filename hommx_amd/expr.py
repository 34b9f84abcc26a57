"""Expression coefficients: ``A(x, y)`` written as text, compiled to a small postfix program that the library interprets on the device
(include/hommx_hip.h, HOMMX_COEF_PROGRAM; csrc/coef_program.hip) and this module interprets with NumPy -- the same operations in the same
order on both sides.

The text is parsed with ``ast`` and never evaluated by Python.  Grammar: the names ``x[0..2]`` (macro cell midpoint), ``y[0..d-1]`` (fast
variable) and ``pi``, numeric literals, ``+ - * /``, unary ``-``, ``**`` with a literal integer exponent 0 .. 8, the comparisons
``< <= > >=`` with ``and`` / ``or`` / ``not`` on them, and the calls ``abs min max where(c, a, b) sqrt sin cos tan exp log tanh``.

Because the library can read the expression, its quadrature degree is estimated from the tree by the rules of UFL's degree estimation
(recalled here, UFL is not a dependency): see ``Expression.degree``.
"""

from __future__ import annotations

import ast
import math

import numpy as np

# opcodes of the program (the OP_* of csrc/coef_program.h, which the kernel and the host validation share)
(OP_CONST, OP_X, OP_Y, OP_ADD, OP_SUB, OP_MUL, OP_DIV, OP_NEG, OP_ABS, OP_MIN, OP_MAX, OP_LT, OP_LE, OP_GT, OP_GE, OP_AND, OP_OR, OP_NOT,
 OP_SELECT, OP_SQRT, OP_SIN, OP_COS, OP_TAN, OP_EXP, OP_LOG, OP_TANH, OP_DUP, OP_STORE) = range(28)
MAX_OPS, MAX_CONSTS, MAX_STACK, MAX_COMP = 128, 32, 16, 6
MAX_POWER = 8

_BINARY = {ast.Add: OP_ADD, ast.Sub: OP_SUB, ast.Mult: OP_MUL, ast.Div: OP_DIV}
_COMPARE = {ast.Lt: OP_LT, ast.LtE: OP_LE, ast.Gt: OP_GT, ast.GtE: OP_GE}
_MATH = {"sqrt": OP_SQRT, "sin": OP_SIN, "cos": OP_COS, "tan": OP_TAN, "exp": OP_EXP, "log": OP_LOG, "tanh": OP_TANH}
_MATH_NUMPY = {OP_SQRT: np.sqrt, OP_SIN: np.sin, OP_COS: np.cos, OP_TAN: np.tan, OP_EXP: np.exp, OP_LOG: np.log, OP_TANH: np.tanh}
# what an instruction takes from the stack and leaves on it
_POPS = {OP_CONST: 0, OP_X: 0, OP_Y: 0, OP_DUP: 1, OP_NEG: 1, OP_ABS: 1, OP_NOT: 1, OP_SELECT: 3, OP_STORE: 1}
_POPS.update({op: 1 for op in _MATH.values()})
_PUSHES = {OP_DUP: 2, OP_STORE: 0}


def _bad(node, why: str):
    what = type(node).__name__
    try:
        what += f" '{ast.unparse(node)}'"
    except Exception:  # pragma: no cover - unparse takes every node the parser makes
        pass
    return ValueError(f"expression: {why}: {what}")


class _Node:
    """One node of the checked tree: ``op`` with ``args`` (nodes) or a leaf (``value``: the constant, or the index of x / y);
    ``boolean``: a comparison or a combination of comparisons; ``degree``: the estimate of the module docstring; ``varying``: depends on
    x or y (a subtree that does not is folded into one constant)."""

    __slots__ = ("op", "args", "value", "boolean", "degree", "varying", "power")

    def __init__(self, op, args=(), value=None, boolean=False, degree=0, varying=False, power=0):
        self.op, self.args, self.value, self.boolean, self.degree, self.varying, self.power = op, tuple(args), value, boolean, degree, varying, power

    def key(self):
        """Structural identity (the off-diagonal texts of a matrix must parse to equal trees)."""
        v = np.float64(self.value).tobytes() if self.op == OP_CONST else self.value
        return (self.op, v, self.power, tuple(a.key() for a in self.args))


_POW = -1  # a node of the tree only: the program spells it DUP / MUL


def _number(node, value) -> _Node:
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise _bad(node, "only numeric literals are allowed")
    return _Node(OP_CONST, value=float(value))


def _check(node) -> _Node:
    """ast node -> checked tree; anything outside the grammar raises ValueError naming the node."""
    if isinstance(node, ast.Constant):
        return _number(node, node.value)
    if isinstance(node, ast.Name):
        if node.id == "pi":
            return _Node(OP_CONST, value=math.pi)
        raise _bad(node, "unknown name (x[i], y[i] and pi are the names)")
    if isinstance(node, ast.Subscript):
        if not (isinstance(node.value, ast.Name) and node.value.id in ("x", "y")):
            raise _bad(node, "only x and y are indexed")
        idx = node.slice
        if not (isinstance(idx, ast.Constant) and isinstance(idx.value, int) and not isinstance(idx.value, bool) and 0 <= idx.value <= 2):
            raise _bad(node, "the index of x and y is a literal 0, 1 or 2")
        fast = node.value.id == "y"
        return _Node(OP_Y if fast else OP_X, value=int(idx.value), degree=1 if fast else 0, varying=True)
    if isinstance(node, ast.UnaryOp):
        a = _check(node.operand)
        if isinstance(node.op, ast.USub):
            return _Node(OP_NEG, [_numeric(a, node)], degree=a.degree, varying=a.varying)
        if isinstance(node.op, ast.UAdd):
            return _numeric(a, node)
        if isinstance(node.op, ast.Not):
            return _Node(OP_NOT, [_logical(a, node)], boolean=True, varying=a.varying)
        raise _bad(node, "unknown unary operator")
    if isinstance(node, ast.BinOp):
        if isinstance(node.op, ast.Pow):
            a = _numeric(_check(node.left), node)
            k = node.right
            if not (isinstance(k, ast.Constant) and isinstance(k.value, int) and not isinstance(k.value, bool) and 0 <= k.value <= MAX_POWER):
                raise _bad(node, f"the exponent of ** is a literal integer 0 .. {MAX_POWER}")
            return _Node(_POW, [a], power=int(k.value), degree=k.value * a.degree, varying=a.varying and k.value > 0)
        if type(node.op) not in _BINARY:
            raise _bad(node, "unknown binary operator")
        a, b = _numeric(_check(node.left), node), _numeric(_check(node.right), node)
        op = _BINARY[type(node.op)]
        degree = max(a.degree, b.degree) if op in (OP_ADD, OP_SUB) else a.degree + b.degree
        return _Node(op, [a, b], degree=degree, varying=a.varying or b.varying)
    if isinstance(node, ast.Compare):
        if len(node.ops) != 1 or type(node.ops[0]) not in _COMPARE:
            raise _bad(node, "a comparison is one of < <= > >= between two values")
        a, b = _numeric(_check(node.left), node), _numeric(_check(node.comparators[0]), node)
        return _Node(_COMPARE[type(node.ops[0])], [a, b], boolean=True, varying=a.varying or b.varying)
    if isinstance(node, ast.BoolOp):
        op = OP_AND if isinstance(node.op, ast.And) else OP_OR
        parts = [_logical(_check(v), node) for v in node.values]
        out = parts[0]
        for p in parts[1:]:  # left to right, as Python evaluates them
            out = _Node(op, [out, p], boolean=True, varying=out.varying or p.varying)
        return out
    if isinstance(node, ast.Call):
        if not isinstance(node.func, ast.Name) or node.keywords:
            raise _bad(node, "unknown call")
        name, args = node.func.id, [_check(a) for a in node.args]
        varying = any(a.varying for a in args)
        if name == "abs" and len(args) == 1:
            return _Node(OP_ABS, [_numeric(args[0], node)], degree=args[0].degree, varying=varying)
        if name in ("min", "max") and len(args) == 2:
            a, b = _numeric(args[0], node), _numeric(args[1], node)
            return _Node(OP_MIN if name == "min" else OP_MAX, [a, b], degree=max(a.degree, b.degree), varying=varying)
        if name == "where" and len(args) == 3:
            c, a, b = _logical(args[0], node), _numeric(args[1], node), _numeric(args[2], node)
            return _Node(OP_SELECT, [c, a, b], degree=max(a.degree, b.degree), varying=varying)  # the condition does not count
        if name in _MATH and len(args) == 1:
            a = _numeric(args[0], node)
            return _Node(_MATH[name], [a], degree=0 if a.degree == 0 else a.degree + 2, varying=varying)
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


def _parse(text) -> _Node:
    if isinstance(text, (int, float)) and not isinstance(text, bool):
        text = repr(float(text))
    if not isinstance(text, str):
        raise ValueError(f"expression: a component is a text; got {type(text).__name__}")
    try:
        tree = ast.parse(text.strip(), mode="eval")
    except SyntaxError as e:
        raise ValueError(f"expression: cannot parse {text!r}: {e.msg}") from None
    return _numeric(_check(tree.body), tree.body)


def _emit(n: _Node, ops: list, consts: list):
    """Postfix code of a tree.  A subtree without x and y is one constant: the value this module's own interpreter gives it, so literals
    fold exactly where Python's evaluation order brings two of them together (``2*pi*y[0]`` holds the constant 2 pi; ``y[0]*2*pi`` none)."""
    if not n.varying and not n.boolean:
        if n.op == OP_CONST:
            value = n.value
        else:
            sub_ops, sub_consts = [], []
            _emit_plain(n, sub_ops, sub_consts)
            sub_ops.append((OP_STORE, 0))
            with np.errstate(all="ignore"):
                value = float(np.asarray(_run(sub_ops, sub_consts, 1, np.zeros((3, 1)), np.zeros((3, 1)))[0]).reshape(-1)[0])
        bits = np.float64(value).tobytes()
        for k, c in enumerate(consts):
            if np.float64(c).tobytes() == bits:
                break
        else:
            k = len(consts)
            consts.append(value)
        ops.append((OP_CONST, k))
        return
    _emit_plain(n, ops, consts)


def _emit_plain(n: _Node, ops: list, consts: list):
    if n.op == OP_CONST:
        consts.append(n.value)
        ops.append((OP_CONST, len(consts) - 1))
    elif n.op in (OP_X, OP_Y):
        ops.append((n.op, n.value))
    elif n.op == _POW:
        if n.power == 0:  # a**0 is 1 whatever a is
            _emit(_Node(OP_CONST, value=1.0), ops, consts)
            return
        _emit(n.args[0], ops, consts)
        ops.extend([(OP_DUP, 0)] * (n.power - 1))  # a a ... a, then the products: ((a a) a) a up to the order of commuting factors
        ops.extend([(OP_MUL, 0)] * (n.power - 1))
    else:
        for a in n.args:
            _emit(a, ops, consts)
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


def _run(ops, consts, n_comp: int, x, y) -> list:
    """Interpret a program with NumPy on x[3, ...] and y[d, ...] (broadcast against each other): one array per component, each operation
    the separately rounded IEEE operation the kernel performs."""
    stack, out = [], [None] * n_comp
    one, zero = np.float64(1.0), np.float64(0.0)
    flag = lambda m: np.where(m, one, zero)
    for op, k in ops:
        if op == OP_CONST:
            stack.append(np.float64(consts[k]))
        elif op == OP_X:
            stack.append(np.asarray(x[k], dtype=np.float64))
        elif op == OP_Y:
            stack.append(np.asarray(y[k], dtype=np.float64))
        elif op == OP_DUP:
            stack.append(stack[-1])
        elif op == OP_STORE:
            out[k] = stack.pop()
        elif op == OP_SELECT:
            b, a, c = stack.pop(), stack.pop(), stack.pop()
            stack.append(np.where(c != 0.0, a, b))
        elif op in (OP_NEG, OP_ABS, OP_NOT) or op in _MATH_NUMPY:
            a = stack.pop()
            stack.append(-a if op == OP_NEG else np.abs(a) if op == OP_ABS else flag(a == 0.0) if op == OP_NOT else _MATH_NUMPY[op](a))
        else:
            b, a = stack.pop(), stack.pop()
            if op == OP_ADD:
                v = a + b
            elif op == OP_SUB:
                v = a - b
            elif op == OP_MUL:
                v = a * b
            elif op == OP_DIV:
                v = a / b
            elif op == OP_MIN:
                v = np.where(b < a, b, a)
            elif op == OP_MAX:
                v = np.where(b > a, b, a)
            elif op == OP_LT:
                v = flag(a < b)
            elif op == OP_LE:
                v = flag(a <= b)
            elif op == OP_GT:
                v = flag(a > b)
            elif op == OP_GE:
                v = flag(a >= b)
            elif op == OP_AND:
                v = flag((a != 0.0) & (b != 0.0))
            elif op == OP_OR:
                v = flag((a != 0.0) | (b != 0.0))
            else:
                raise ValueError(f"program: unknown opcode {op}")
            stack.append(v)
    return out


class Expression:
    """A coefficient ``A(x, y)`` given as text (module docstring: the grammar).

    ``Expression(text)`` is a scalar coefficient (the Poisson classes), ``Expression(lam=..., mu=...)`` a ``Lame`` pair (the elasticity
    classes), ``Expression([[a, b], [b, c]])`` a symmetric d x d matrix (the Poisson classes; the two texts of an off-diagonal entry must
    parse to equal trees).  Passing one as ``A`` lets the solver classes sample on the DEVICE: the points of the micro quadrature rule go
    once, three numbers per macro cell (its midpoint) after them, and a bytecode kernel forms the element means.

    ``degree``: the quadrature degree of the expression, estimated from its tree by UFL's rules -- a literal, ``x[i]`` and ``pi`` 0;
    ``y[i]`` 1; a sum or difference the larger; a product or quotient the sum; ``a**k`` k times; ``abs`` keeps; ``where`` / ``min`` /
    ``max`` the larger of the values (not the condition); a math function 0 of an argument of degree 0, else the argument's + 2.  (UFL is
    not installed where this is developed: the rules are recalled, not run.)  Several components: the largest.

    The object is also a plain callable ``A(x, y)`` -- it interprets ``program()`` with NumPy --, so every generic path accepts it.
    ``host_stream`` is the documented host equivalent of the device sampler: the same IEEE operations in the same order.
    """

    def __init__(self, text=None, *, lam=None, mu=None):
        if (lam is None) != (mu is None) or (text is None) == (lam is None):
            raise ValueError("Expression(text), Expression([[a, b], [b, c]]) or Expression(lam=..., mu=...)")
        self.dim = None  # the d of a matrix
        if lam is not None:
            self.shape, texts = "lame", [lam, mu]
        elif isinstance(text, (list, tuple)):
            d = len(text)
            if d not in (2, 3) or any(not isinstance(r, (list, tuple)) or len(r) != d for r in text):
                raise ValueError("expression: a matrix is 2 x 2 or 3 x 3")
            self.shape, self.dim = "matrix", d
            pairs = [(0, 0), (1, 1), (0, 1)] if d == 2 else [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]  # the component order of the ABI
            for i, j in pairs:
                if i != j and _parse(text[i][j]).key() != _parse(text[j][i]).key():
                    raise ValueError(f"expression: the matrix must be symmetric; entries [{i}][{j}] and [{j}][{i}] differ")
            texts, self._pairs = [text[i][j] for i, j in pairs], pairs
        else:
            self.shape, texts = "scalar", [text]
        self.texts = tuple(str(t) for t in texts)
        trees = [_parse(t) for t in texts]
        self.n_comp = len(trees)
        self.degree = max(t.degree for t in trees)
        ops, consts = [], []
        for c, t in enumerate(trees):
            _emit(t, ops, consts)
            ops.append((OP_STORE, c))
        if len(ops) > MAX_OPS:
            raise ValueError(f"expression: too long: {len(ops)} instructions, at most {MAX_OPS}")
        if len(consts) > MAX_CONSTS:
            raise ValueError(f"expression: too many constants: {len(consts)}, at most {MAX_CONSTS}")
        deepest = max(stack_depths(ops))
        if deepest > MAX_STACK:
            raise ValueError(f"expression: too deep: stack depth {deepest}, at most {MAX_STACK}")
        self._ops = np.array(ops, dtype=np.uint8).reshape(-1, 2)
        self._consts = np.array(consts, dtype=np.float64)
        self.n_y = 1 + max([int(k) for op, k in ops if op == OP_Y], default=-1)  # fast-variable components the expression reads

    def program(self) -> tuple[np.ndarray, np.ndarray]:
        """(ops[n_ops, 2] uint8 = (opcode, operand), consts[n_consts] float64): the postfix program of hommx_coef_program -- every
        component's code followed by its ``STORE c``."""
        return self._ops.copy(), self._consts.copy()

    def components(self, x, y) -> list:
        """The components at x[3, ...], y[d, ...], each broadcast to the common shape of x[0] and y[0]."""
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        if self.n_y > y.shape[0]:
            raise ValueError(f"the expression reads y[{self.n_y - 1}]; the fast variable has {y.shape[0]} components")
        shape = np.broadcast(x[0], y[0]).shape
        with np.errstate(all="ignore"):
            out = _run(self._ops.tolist(), self._consts, self.n_comp, x, y)
        return [np.broadcast_to(v, shape) for v in out]

    def __call__(self, x, y):
        v = self.components(x, y)
        if self.shape == "scalar":
            return np.array(v[0])
        if self.shape == "lame":
            from .hmm import Lame

            return Lame(np.array(v[0]), np.array(v[1]))
        out = np.empty(v[0].shape + (self.dim, self.dim))
        for c, (i, j) in enumerate(self._pairs):
            out[..., i, j] = out[..., j, i] = v[c]
        return out

    def host_stream(self, x: np.ndarray, yq: np.ndarray, w: np.ndarray) -> np.ndarray:
        """Element means coef[N, n_el(, n_comp)] at the midpoints x[N, 3] from the points yq[n_el, n_q, d] and weights w[n_q], exactly as
        the device forms them: ``acc = acc + w[q] * v_q`` with q ascending, from 0."""
        x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
        n_el, nq, d = yq.shape
        acc = [np.zeros((x.shape[0], n_el)) for _ in range(self.n_comp)]
        for q in range(nq):
            v = self.components(x.T[:, :, None], np.moveaxis(yq[:, q, :], -1, 0)[:, None, :])
            for c in range(self.n_comp):
                acc[c] = acc[c] + w[q] * v[c]
        return acc[0] if self.n_comp == 1 else np.stack(acc, axis=-1)
