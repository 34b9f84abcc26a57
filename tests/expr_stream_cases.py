"""The programs and batch shapes of tests/golden/expr_streams/expr_streams_parent.npz: what tools/record_expr_streams.py records on the
commit before the interpreter kernels of csrc/coef_program.hip became one template, and what tests/test_gpu_expr_parent_bits.py
replays.

Every program goes through ``MicroCellPlan.expand`` -- the value pass, whatever slots it has -- and, where it has differentiable
slots, through ``MicroCellPlan.expand_tangents``.  Between them the programs hold every opcode; every tangent rule once with a live
tangent and once with a dead one (a block of rules reads ONE slot: it is live in that slot and dead in every other, and ``p1_dead``
reads none); SIN and COS of an argument without a parameter; a square root of zero and a division by zero that no slot reaches; a
stack of depth 16; and 1, 2, 3 and 4 slots as parameters only, fields only and mixed.

Shapes: 9 cells of the 4 x 4 micro mesh (32 elements) with the rule of degree 3 are 288 threads -- 2, 3 and 5 blocks of 256, 128 and 64
threads, each with a tail; 2 cells of the matrix-valued 3 x 3 x 3 mesh (162 elements, 324 threads; the library admits no
smaller n_micro) run six components and ``STORE 5``.
hommx_amd is imported inside the functions: the recording tool chooses the tree first.
"""

import numpy as np

QUADRATURE_DEGREE = 3


def _rules_a(s):
    return f"sqrt({s} + y[0]) + sin({s}*y[0]) + cos({s} - y[1]) + tan(0.5*{s}*y[0])"


def _rules_b(s):
    return f"exp(-{s}*y[1]) + log({s} + y[1]) + tanh({s}*y[0] - 0.5) + abs({s}*(y[0] - 0.5))"


def _rules_c(s):
    return f"min({s}*y[0], 0.3) + max({s}*y[1], 0.4) + where(y[0] < 0.5, {s}, x[0]) + x[1]/(1 + {s}*y[1])"


def _logic(s):  # every comparison, AND, OR, NOT, and DUP
    return (f"where(abs(y[0] - 0.5) <= 0.25 or y[1] >= 0.875, {s}, 1) + where(y[0] > 0.5 and not y[1] < 0.25, 1, -{s}/8)"
            f" + ({s} + y[0])**3")


def _blocks(a, b, c):
    return f"{_rules_a(a)} + {_rules_b(b)} + {_rules_c(c)}"


def _deep(leaves):
    """a0 + (a1 * (a2 + (a3 * ...))): the right operand is evaluated last, so the stack holds every leaf at once."""
    text = leaves[-1]
    for k in range(len(leaves) - 2, -1, -1):
        text = f"{leaves[k]} {'+' if k % 2 == 0 else '*'} ({text})"
    return text


NO_SLOT = "(0.5 + x[2])"  # in [0.5, 1.5] like a parameter or a field of these cases, and reads neither
ZEROS = "sqrt(y[0] - y[0]) + min(1/(y[1] - y[1]), 2)"  # sqrt(0), 1/0: rules that give NaN unless a dead tangent skips them
WAVE = "sin(2*pi*y[0])*cos(2*pi*y[1])"  # SIN and COS of an argument without a parameter

# name -> (text, p or None, number of fields); the slots are the parameters, then the fields; p and f lie in [0.5, 1.5]
SCALAR = {
    "none": (f"{_logic('x[1]')} + {WAVE}", None, 0),
    "p1": (_blocks("p[0]", "p[0]", "p[0]"), [0.75], 0),
    "p1_dead": (f"p[0] + {_blocks(NO_SLOT, NO_SLOT, NO_SLOT)} + {ZEROS}", [0.75], 0),
    "p2": (f"{_blocks('p[0]', 'p[1]', 'p[0]')} + {_logic('p[1]')}", [0.75, 1.25], 0),
    "p3": (f"{_blocks('p[0]', 'p[1]', 'p[2]')} + {ZEROS}", [0.75, 1.25, 0.625], 0),
    "p4": (f"{_blocks('p[0]', 'p[1]', 'p[2]')} + p[3]*{WAVE}", [0.75, 1.25, 0.625, 1.375], 0),
    "f1": (_blocks("f[0]", "f[0]", "f[0]"), None, 1),
    "f2": (f"{_blocks('f[0]', 'f[1]', 'f[0]')} + f[1]*{WAVE}", None, 2),
    "f3": (f"{_blocks('f[0]', 'f[1]', 'f[2]')} + {ZEROS}", None, 3),
    "f4": (f"{_blocks('f[0]', 'f[1]', 'f[2]')} + f[3]*{WAVE}", None, 4),
    "p1f1": (f"{_blocks('p[0]', 'f[0]', 'p[0]')} + {_logic('f[0]')}", [0.75], 1),
    "p1f2": (f"{_blocks('f[1]', 'p[0]', 'f[0]')} + {ZEROS}", [1.25], 2),
    "p2f2": (f"{_blocks('f[1]', 'p[1]', 'f[0]')} + p[0]*{WAVE}", [0.75, 1.25], 2),
    "deep_p1": (_deep(["p[0]", "y[0]", "x[0]", "y[1]", "p[0]", "x[1]", "y[0]", "x[2]"] * 2), [0.75], 0),
    "deep_p1f3": (_deep(["p[0]", "y[0]", "f[0]", "y[1]", "x[0]", "f[1]", "y[0]", "x[1]", "f[2]", "y[1]", "x[2]", "y[0]", "p[0]", "y[1]",
                         "f[0]", "y[0]"]), [0.75], 3),
}

# the six components of a symmetric 3 x 3 matrix: STORE 0 .. 5, two slots
_OFF = ["0.25*x[1]*f[0]*y[2]", "0.125*p[0]*sin(2*pi*y[2])", "x[0]/(4 + f[0]*y[1])"]  # [0][1], [0][2], [1][2]
MATRIX_3D = ([[f"2 + p[0]*y[0]*y[2] + sqrt(f[0] + y[1])", _OFF[0], _OFF[1]],
              [_OFF[0], f"3 + exp(-f[0]*y[2]) + {ZEROS}", _OFF[2]],
              [_OFF[1], _OFF[2], f"4 + tanh(p[0]*y[2] - 0.5) + cos(2*pi*y[0])"]], [0.75], 1)

# name -> (dim, n_micro, kind, cells)
SHAPES = {"scalar": (2, 4, "poisson", 9), "matrix": (3, 3, "poisson_matrix", 2)}


def cases():
    """[(name, shape name, Expression)] in recording order."""
    from hommx_amd import hmm

    out = [(name, "scalar", hmm.Expression(text, p=p, fields=n_fields or None)) for name, (text, p, n_fields) in SCALAR.items()]
    text, p, n_fields = MATRIX_3D
    return out + [("matrix3d", "matrix", hmm.Expression(text, p=p, fields=n_fields))]


def plan(shape):
    from hommx_amd import MicroCellPlan

    dim, n, kind, _ = SHAPES[shape]
    return MicroCellPlan(dim, n, kind)


def stream(shape, A):
    """The CoefStream of expression A on the shape: the rule of degree 3, midpoints in [0, 1]^3 and field values in [0.5, 1.5], all
    different from cell to cell."""
    from hommx_amd import hmm, mesh as Mm
    from hommx_amd.batch import CoefStream

    dim, n, _, nc = SHAPES[shape]
    micro = Mm.create_unit_square(n, n) if dim == 2 else Mm.create_unit_cube(n, n, n)
    bary, w = hmm.micro_quadrature(dim, QUADRATURE_DEGREE)
    yq = np.ascontiguousarray(np.einsum("qa,eak->eqk", bary, micro.cell_vertices()))
    rng = np.random.default_rng(20)
    rows = np.ascontiguousarray(np.concatenate([rng.uniform(0.0, 1.0, (nc, 3)), rng.uniform(0.5, 1.5, (nc, A.n_fields))], axis=1))
    return CoefStream.program(yq, np.ascontiguousarray(w), *A.program(), A.n_comp, rows, n_params=A.n_params, n_fields=A.n_fields)
