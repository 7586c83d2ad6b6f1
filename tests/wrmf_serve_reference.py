"""numpy fp64 restatement of the sparse WRMF objective (include/dcue.h dcue_wrmf_objective) and the
shared problems of the WRMF serving tests.

With s_ui = x_u . y_i, c_ui = 1 + alpha v_ui on the observed pairs:
  L = sum_{observed} [c_ui (1 - s_ui)^2 - s_ui^2] + sum_{a,b} (X^T X)_ab (Y^T Y)_ab + lam (tr X^T X + tr Y^T Y)
which equals oracle.wrmf_oracle.objective (the dense sum over every pair) because the sum of s_ui^2 over
ALL pairs is the Frobenius inner product of the two Gram matrices."""
import numpy as np


def objective_terms(X, Y, rows, cols, values, alpha, lam):
    """(L, observed term, all-pairs term, regulariser), fp64; `amplification` below needs them."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    v = np.ones(len(rows)) if values is None else np.asarray(values, dtype=np.float64)
    s = np.einsum("pk,pk->p", X[rows], Y[cols]) if len(rows) else np.zeros(0)
    observed = float(((1.0 + alpha * v) * (1.0 - s) ** 2 - s * s).sum())
    gx, gy = X.T @ X, Y.T @ Y
    all_pairs = float((gx * gy).sum())
    reg = float(lam * (np.trace(gx) + np.trace(gy)))
    return observed + all_pairs + reg, observed, all_pairs, reg


def amplification(X, Y, rows, cols, values, alpha, lam):
    """A = (sum |observed terms| + sum |G_X o G_Y| + regulariser) / L: how much larger the summed
    magnitudes are than the result, i.e. what a relative rounding error of the sums is multiplied by."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    v = np.ones(len(rows)) if values is None else np.asarray(values, dtype=np.float64)
    s = np.einsum("pk,pk->p", X[rows], Y[cols]) if len(rows) else np.zeros(0)
    mag = float(np.abs((1.0 + alpha * v) * (1.0 - s) ** 2 - s * s).sum())
    gx, gy = X.T @ X, Y.T @ Y
    mag += float(np.abs(gx * gy).sum()) + float(lam * (np.trace(gx) + np.trace(gy)))
    return mag / objective_terms(X, Y, rows, cols, values, alpha, lam)[0]


def problem(seed, n_users, n_items, d, with_values, density=0.08, empty_user=None, empty_item=None):
    """Distinct random (user, item) pairs sorted by user (the by-user CSR order), optional play counts
    in 1..20, and N(0, 0.1) fp32 factors. empty_user / empty_item: a row / column left without pairs."""
    rs = np.random.RandomState(seed)
    pick = rs.rand(n_users, n_items) < density
    if n_users * n_items == 1:
        pick[:] = True
    if empty_user is not None:
        pick[empty_user] = False
    if empty_item is not None:
        pick[:, empty_item] = False
    rows, cols = np.nonzero(pick)
    values = rs.randint(1, 21, len(rows)).astype(np.float32) if with_values else None
    X = (rs.randn(n_users, d) * 0.1).astype(np.float32)
    Y = (rs.randn(n_items, d) * 0.1).astype(np.float32)
    return dict(rows=rows.astype(np.int64), cols=cols.astype(np.int64), values=values, X=X, Y=Y,
                n_users=n_users, n_items=n_items, d=d)


def als_iterations(p, alpha, lam, n):
    """n oracle ALS iterations (users, then items) from the problem's factors: (X, Y) fp32."""
    from oracle import wrmf_oracle as W
    X, Y = p["X"].astype(np.float64), p["Y"].astype(np.float64)
    by_user = W.csr(p["rows"], p["cols"], p["values"], p["n_users"])
    by_item = W.csr(p["cols"], p["rows"], p["values"], p["n_items"])
    for _ in range(n):
        X = W.half_step(Y, *by_user, alpha, lam)
        Y = W.half_step(X, *by_item, alpha, lam)
    return X.astype(np.float32), Y.astype(np.float32)
