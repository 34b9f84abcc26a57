"""Test-side NumPy restatement of the load solve of the frontal mesh route ("load solves"; k_mesh_front_rhs of
hommx_amd/csrc/mesh_front.hip): the record the elimination leaves -- every pivot's column before its update -- and the forward and
backward pass over it, for any kind on any periodic mesh, on top of ``loads_ref.Cell``.

    record    K of the cell (dof = node * bs + component) eliminated node by node in `order`, component by component; the last node of
              the order is pinned: its rows and columns never enter.  A pivot's column is stored before the update; the update clears the
              pivot's row and column, so the rows of unknowns eliminated earlier (those of the same node among them) are stored as zeros.
    forward   r = -f with zeros at the pinned node; per pivot p in elimination order: y = r[p], r[i] -= col[i] (y / d) for i != p
    backward  pivots in reverse: x[p] = (y[p] - sum_{i != p} col[i] x[i]) / d; the pinned node keeps 0; the mean removed per component

tests/test_mesh_front_loads_host.py holds the passes to ``loads_ref.Cell.solve``.
"""

from __future__ import annotations

import numpy as np


def dense_stiffness(cell) -> np.ndarray:
    """K of a ``loads_ref.Cell``, dense, dof = node * bs + component."""
    nl = cell.rows.shape[1]
    Ke = np.einsum("e,eta,etu,eub->eab", cell.vol, cell.B, cell.V, cell.B)
    K = np.zeros((cell.nd, cell.nd))
    np.add.at(K, (np.repeat(cell.rows, nl, axis=1).ravel(), np.tile(cell.rows, (1, nl)).ravel()), Ke.ravel())
    return K


def factor(K: np.ndarray, order, bs: int) -> list:
    """[(p, column[nd])] in elimination order: the record of ``K`` for the node order ``order`` (its last node pinned)."""
    order = np.asarray(order)
    S = np.array(K, dtype=float)
    pinned = order[-1] * bs + np.arange(bs)
    S[pinned, :] = 0.0
    S[:, pinned] = 0.0
    record = []
    for node in order[:-1]:
        for c in range(bs):
            p = int(node) * bs + c
            col = S[:, p].copy()
            assert col[p] > 0.0
            record.append((p, col))
            S -= np.outer(col, col / col[p])
            S[p, :] = 0.0
            S[:, p] = 0.0
    return record


def correctors(record: list, f: np.ndarray, order, bs: int) -> np.ndarray:
    """chi[l, nd] of K chi_l = -f[l] by the two passes over ``record``, mean-free per component."""
    order = np.asarray(order)
    r = -np.array(f, dtype=float)
    r[:, order[-1] * bs + np.arange(bs)] = 0.0
    for p, col in record:
        y = r[:, p].copy()
        for i in np.flatnonzero(col):
            if i != p:
                r[:, i] -= col[i] * (y / col[p])
    for p, col in reversed(record):
        rows = np.flatnonzero(col)
        rows = rows[rows != p]
        r[:, p] = (r[:, p] - r[:, rows] @ col[rows]) / col[p]
    x = r.reshape(len(r), -1, bs)
    return (x - x.mean(axis=1, keepdims=True)).reshape(len(r), -1)


def same_node_rows_cleared(record: list, bs: int) -> int:
    """How many stored entries are rows of an earlier unknown of the pivot's own node (all must be zero: the elimination cleared them)."""
    count = 0
    for p, col in record:
        for q in range(p - p % bs, p):
            assert col[q] == 0.0
            count += 1
    return count
